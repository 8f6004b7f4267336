"""The host side of every gather of the fitting stack (csrc/md_gather.h): the CSR of codes sorted stably by the row they name."""
import torch

from . import _lib

INT32_MAX = 2 ** 31 - 1


def csr_by_row(dest, n_rows):
    """dest integer [K] or [B,K] with values in [0, n_rows), not checked: code k names row dest[k].  Returns (ptr int32
    [n_rows + 1] or [B, n_rows + 1], order int32 of dest's shape), both contiguous: order holds the codes sorted stably by row
    (ascending inside a row) and ptr[r]:ptr[r + 1] is the span of row r in it.  Torch plumbing on dest's device, the CPU included."""
    K = dest.shape[-1]
    if K > INT32_MAX or n_rows >= INT32_MAX:
        raise _lib.MeshDiffusionHipError(f"the {K} codes and {n_rows} rows of a gather must fit int32 (MD_ERR_UNSUPPORTED)")
    vals, order = torch.sort(dest, dim=-1, stable=True)
    bounds = torch.arange(n_rows + 1, dtype=dest.dtype, device=dest.device)
    if dest.dim() == 2:
        bounds = bounds.expand(dest.shape[0], -1).contiguous()
    ptr = torch.searchsorted(vals.contiguous(), bounds)
    return ptr.to(torch.int32).contiguous(), order.to(torch.int32).contiguous()


def check_faces(faces, n_verts, what, limits=None, not_triangles=ValueError):
    """faces [F,3] -> int64 contiguous with every index in [0, n_verts): checked once, with one aminmax, on the tensor's own device.
    `limits(F)` raises what the caller refuses beyond that, after the shape check and before the conversion; `what` heads the messages."""
    if faces.dim() != 2 or faces.shape[-1] != 3:
        raise not_triangles(f"{what}: expected faces [F,3], got {tuple(faces.shape)}")
    if limits is not None:
        limits(faces.shape[0])
    f = faces.to(torch.int64).contiguous()
    if f.shape[0] > 0:
        lo, hi = torch.aminmax(f)
        if int(lo) < 0 or int(hi) >= n_verts:
            raise ValueError(f"{what}: faces name vertices outside [0, {n_verts})")
    return f
