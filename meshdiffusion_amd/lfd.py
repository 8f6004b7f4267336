"""Light-field distance for the generation metrics on MI355X -- host side of csrc/lfd.hip.

The paper behind the reference reports MMD / COV / 1-NNA under two distances, the chamfer distance and the light-field distance
(LFD) of Chen, Tian, Shen and Ouhyoung 2003.  LFD looks at the surface AS RENDERED: a model is seen from the vertices of a
regular dodecahedron (one silhouette per antipodal vertex pair: 10 of them make a light field), every silhouette becomes a
small descriptor (35 Zernike moment magnitudes of the region, 10 Fourier magnitudes of its angular signature), and the
distance of two models is the smallest sum of the ten image distances over the pairs of light fields and the 60 rotations of
the dodecahedron.  L = 10 light fields per model, the dodecahedron turned a little differently for each, make up for the
coarse set of rotations.

This module is LFD IN THE MANNER OF that method, by THE LFD CONTRACT in the header comment of csrc/lfd.hip (restated in float64
by tests/lfd_cases.py).  The original executable traces contours and scales its coefficients in its own way; no implementation
was consulted, and the values here are NOT comparable with numbers produced by that executable -- only with each other.

    silhouettes      the L x 10 orthographic silhouettes of a mesh, from the rasteriser (`render.rasterize(num_layers=1)`)
    describe         md_lfd_describe: one 48-byte descriptor per silhouette
    lfd_descriptors  both, over a list of meshes: uint8 [M, L, 10, 48]
    lfd_matrix       md_lfd_matrix: the all-pairs int32 matrix (exact integers; the triangular launch for a union)
    lfd_metrics      MMD / COV / 1-NNA from one union matrix through `metrics.mmd_cov` / `metrics.one_nna`

`view_directions`, `rotation_perms` and `field_rotations` are float64 numpy on the host.  The kernels run on the GPU only: a CPU
tensor is an error, not a fallback.  Not built: contour tracing and parity with the original executable, gradients, batching
several meshes into one rasteriser call, a multi-GPU split of the matrix.
"""
import functools
import math

import numpy as np
import torch

from . import _lib
from .hip_ops import call

VIEWS = _lib.LFD_VIEWS                    # silhouettes per light field
DESC_BYTES = _lib.LFD_DESC_BYTES          # 35 Zernike + 10 Fourier + 3 zero bytes
COEFS = _lib.LFD_COEFS
MAX_RES = _lib.LFD_MAX_RES
MAX_FIELDS = _lib.LFD_MAX_FIELDS
MAX_ROTATIONS = _lib.LFD_MAX_ROTATIONS
RUN = _lib.LFD_RUN                        # y models per workgroup of md_lfd_matrix
FIELD_CONSTANTS = (0.8191725134, 0.6710436067, 0.5497004779)


# ---- the dodecahedron --------------------------------------------------------------------------------------------------------------
def _vertices():
    """The 20 vertices (+-1, +-1, +-1), (0, +-1/phi, +-phi) and the cyclic shifts of the latter, float64 [20,3]."""
    phi = (1 + math.sqrt(5)) / 2
    v = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    for a in (1, -1):
        for b in (1, -1):
            p = (0.0, a / phi, b * phi)
            v += [p, (p[2], p[0], p[1]), (p[1], p[2], p[0])]
    return np.array(v, dtype=np.float64)


def view_directions():
    """float64 [10,3]: one unit vector per antipodal vertex pair of the dodecahedron -- of each pair the vertex whose first
    non-zero coordinate is positive, in the order
        (1,1,1) (1,1,-1) (1,-1,1) (1,-1,-1)   (0,1/phi,phi) (0,1/phi,-phi)   (phi,0,1/phi) (phi,0,-1/phi)   (1/phi,phi,0) (1/phi,-phi,0)
    over sqrt(3).  A silhouette seen along d is the mirror image of the one seen along -d, and the descriptor does not see the
    difference, so ten views stand for the twenty vertices."""
    phi = (1 + math.sqrt(5)) / 2
    d = np.array([(1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (0, 1 / phi, phi), (0, 1 / phi, -phi), (phi, 0, 1 / phi),
                  (phi, 0, -1 / phi), (1 / phi, phi, 0), (1 / phi, -phi, 0)], dtype=np.float64)
    return d / math.sqrt(3.0)


def _axis_rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


@functools.lru_cache(maxsize=None)
def _group():
    """(rotations float64 [60,3,3], perms uint8 [60,10]): the closure of a 5-fold rotation (about the face centre (0, phi, 1)) and
    a 3-fold rotation (about the vertex (1, 1, 1)), the identity first, in breadth-first order of the products."""
    phi = (1 + math.sqrt(5)) / 2
    gens = [_axis_rotation((0.0, phi, 1.0), 2 * math.pi / 5), _axis_rotation((1.0, 1.0, 1.0), 2 * math.pi / 3)]
    verts = _vertices()
    for g in gens:                                                               # a generator maps the vertex set onto itself
        if np.abs((verts @ g.T)[:, None] - verts[None]).max(axis=2).min(axis=1).max() > 1e-9:
            raise AssertionError("rotation_perms: a generator does not preserve the dodecahedron")
    found = [np.eye(3)]
    k = 0
    while k < len(found):
        for g in gens:
            cand = g @ found[k]
            if all(np.abs(cand - f).max() > 1e-9 for f in found):
                found.append(cand)
        k += 1
    if len(found) != 60:
        raise AssertionError(f"rotation_perms: the closure has {len(found)} elements, not 60")
    d = view_directions()
    perms = np.zeros((60, VIEWS), dtype=np.uint8)
    for k, g in enumerate(found):
        dots = np.abs((d @ g.T) @ d.T)                                           # |<g d_v, d_u>| = 1 for exactly one u
        perms[k] = dots.argmax(axis=1)
        if dots.max(axis=1).min() < 1 - 1e-9:
            raise AssertionError("rotation_perms: a rotated direction matches no vertex pair")
    return np.stack(found), perms


def rotation_perms():
    """uint8 [60,10]: perm[g][v] = the vertex pair that rotation g of the dodecahedron takes pair v to.  Row 0 is the identity; the
    rows are the 60 rotations (a group: closed under composition and inverse), built in float64 by closing a 5-fold and a 3-fold
    generator and matching the rotated vertices.  A copy: the caller may write to it."""
    return _group()[1].copy()


def rotation_matrices():
    """float64 [60,3,3]: the rotations whose action `rotation_perms` tabulates, in the same order."""
    return _group()[0].copy()


def field_rotations(L=10):
    """float64 [L,3,3]: how the dodecahedron of light field k is turned.  Field 0 is the identity, field k is Rz(a) Ry(b) Rx(c)
    with (a, b, c) = 2 pi frac(k (0.8191725134, 0.6710436067, 0.5497004779)): closed form, no RNG.  For L = 10 every two fields
    are more than 5 degrees apart modulo the 60 rotations (tests/test_cpu_lfd_host.py)."""
    L = int(L)
    if not 1 <= L <= MAX_FIELDS:
        raise ValueError(f"field_rotations: L must be in [1, {MAX_FIELDS}], got {L}")
    out = np.zeros((L, 3, 3), dtype=np.float64)
    for k in range(L):
        a, b, c = (2 * math.pi * math.fmod(k * f, 1.0) for f in FIELD_CONSTANTS)
        out[k] = _axis_rotation((0, 0, 1), a) @ _axis_rotation((0, 1, 0), b) @ _axis_rotation((1, 0, 0), c)
    return out


def view_frames():
    """float64 [10,3,3]: the camera of direction d = view_directions()[v], rows (right, up, d).  The up vector is fixed per
    direction: right = normalise(a x d) with a = e_z, or e_x where |d_z| > 0.9 (the two directions (0, 1/phi, +-phi)), and up = d x
    right.  Another choice turns the silhouette in its plane, which the descriptor does not see (up to pixelisation)."""
    frames = np.zeros((VIEWS, 3, 3), dtype=np.float64)
    for v, d in enumerate(view_directions()):
        a = np.array([1.0, 0.0, 0.0]) if abs(d[2]) > 0.9 else np.array([0.0, 0.0, 1.0])
        right = np.cross(a, d)
        right /= np.linalg.norm(right)
        frames[v] = np.stack([right, np.cross(d, right), d])
    return frames


# ---- silhouettes and descriptors ---------------------------------------------------------------------------------------------------
def _gpu(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.MeshDiffusionHipError(f"{what} runs on the GPU only (no CPU fallback)")


def _resolution(resolution, what):
    R = int(resolution)
    if R < 1:
        raise ValueError(f"{what}: resolution must be positive, got {resolution}")
    if R > MAX_RES:
        raise _lib.MeshDiffusionHipError(f"{what}: resolution {R} exceeds {MAX_RES} (MD_ERR_UNSUPPORTED)")
    return R


def silhouettes(verts, faces, resolution=256, L=10):
    """verts [V,3], faces [F,3] on the GPU -> uint8 [L * 10, R, R], silhouette (k, v) at index 10 k + v: the mesh turned by
    field_rotations(L)[k], seen along view_directions()[v] with the camera of `view_frames`.

    The mesh is centred on the centre of the bounding box of the vertices its faces name and scaled so that the farthest of
    them is at distance 1.  The views are orthographic with half-width 1: pos_clip = (right . p, up . p, d . p / 2, 1), so w = 1
    and z stays inside (-1, 1).  Rasterised by `render.rasterize(num_layers=1)` in calls of at most `render.MAX_VIEWS` views; a
    pixel is set where the face id `rast[..., 3]` is positive.  A mesh without faces, or without extent, is a ValueError."""
    from . import render
    _gpu(verts, "silhouettes")
    R = _resolution(resolution, "silhouettes")
    rot = field_rotations(L)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"silhouettes: expected verts [V,3] and faces [F,3], got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if faces.shape[0] == 0 or verts.shape[0] == 0:
        raise ValueError("silhouettes: the mesh has no faces")
    dev = verts.device
    f = faces.to(dev).to(torch.int64).contiguous()
    if int(f.min()) < 0 or int(f.max()) >= verts.shape[0]:
        raise ValueError("silhouettes: a face index outside the vertices")
    v = verts.detach().to(torch.float32)
    used = v[torch.unique(f)]
    if not bool(torch.isfinite(used).all()):
        raise ValueError("silhouettes: a non-finite vertex")
    centre = (used.min(dim=0).values + used.max(dim=0).values) / 2
    radius = float((used - centre).norm(dim=1).max())
    if radius <= 0:
        raise ValueError("silhouettes: the mesh has no extent")
    p = (v - centre) / radius
    cams = np.einsum("vab,kbc->kvac", view_frames(), rot).reshape(-1, 3, 3)      # camera (k, v) = frame_v . field_k
    cams[:, 2] *= 0.5                                                            # z = d . p / 2
    cams = torch.from_numpy(cams).to(device=dev, dtype=torch.float32)
    out = torch.empty((cams.shape[0], R, R), dtype=torch.uint8, device=dev)
    for lo in range(0, cams.shape[0], render.MAX_VIEWS):
        c = cams[lo:lo + render.MAX_VIEWS]
        xyz = torch.einsum("bac,nc->bna", c, p)
        pos_clip = torch.cat([xyz, torch.ones_like(xyz[..., :1])], dim=-1).contiguous()
        rast = render.rasterize(pos_clip, f, R, num_layers=1)[0]
        out[lo:lo + c.shape[0]] = (rast[..., 3] > 0).to(torch.uint8)
    return out


def describe(masks, return_info=False):
    """masks uint8 (or bool) [n,R,R] on the GPU, a pixel set where non-zero, R <= 512 -> desc uint8 [n,48]: md_lfd_describe, 35
    Zernike bytes (n = 1..10, m = n mod 2, .., n), 10 Fourier bytes, three zero bytes.  return_info: (desc, coef float32 [n,45]
    -- the values 512 z, 512 f before they are rounded to bytes --, status int32 [n]: 1 for an empty mask, whose bytes are 0).
    Two runs agree bit for bit."""
    if not torch.is_tensor(masks) or masks.dim() != 3 or masks.shape[0] < 1 or masks.shape[1] != masks.shape[2] or masks.shape[1] < 1:
        raise ValueError(f"describe: expected masks [n,R,R] with n, R >= 1, got {tuple(getattr(masks, 'shape', ()))}")
    if masks.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"describe: masks must be uint8 or bool, got {masks.dtype}")
    n, R = masks.shape[0], _resolution(masks.shape[1], "describe")
    _gpu(masks, "describe")
    m = masks.detach().to(torch.uint8).contiguous()
    desc = torch.empty((n, DESC_BYTES), dtype=torch.uint8, device=m.device)
    status = torch.empty((n,), dtype=torch.int32, device=m.device)
    coef = torch.empty((n, COEFS), dtype=torch.float32, device=m.device) if return_info else None
    call("md_lfd_describe", m, n, R, desc, coef, status)
    return (desc, coef, status) if return_info else desc


def lfd_descriptors(meshes, resolution=256, L=10, skip_empty=False):
    """meshes: a list of (verts [V,3], faces [F,3]) -- tensors or arrays; anything not already on a GPU is moved to the current
    one.  Returns (uint8 [M,L,10,48], skipped): `silhouettes` then `describe` per mesh.  A mesh without faces or extent, or whose
    every silhouette is empty, raises a ValueError with its index, or with skip_empty=True is left out and its index listed in
    `skipped` (as `metrics.clouds_from_meshes` does)."""
    out, skipped = [], []
    for k, (verts, faces) in enumerate(meshes):
        why = None
        if min(int(t.numel()) if torch.is_tensor(t) else np.asarray(t).size for t in (verts, faces)) == 0:
            why = "has no faces"                                                 # before anything is moved to a device
        else:
            dev = verts.device if isinstance(verts, torch.Tensor) and verts.is_cuda else torch.device("cuda")
            v = torch.as_tensor(verts, dtype=torch.float32, device=dev).reshape(-1, 3)
            f = torch.as_tensor(faces, device=dev).to(torch.int64).reshape(-1, 3)
            try:
                desc, _, status = describe(silhouettes(v, f, resolution, L), return_info=True)
                if bool((status == 1).all()):
                    why = "has only empty silhouettes"
            except ValueError as e:
                why = str(e).split(": ", 1)[-1]
        if why is not None:
            if not skip_empty:
                raise ValueError(f"lfd_descriptors: mesh {k} {why}")
            skipped.append(k)
            continue
        out.append(desc.reshape(int(L), VIEWS, DESC_BYTES))
    if not out:
        raise ValueError("lfd_descriptors: no mesh with a silhouette")
    return torch.stack(out), skipped


# ---- the matrix and the metrics ----------------------------------------------------------------------------------------------------
def _models(t, what):
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[0] < 1 or t.shape[2] != VIEWS or t.shape[3] != DESC_BYTES:
        raise ValueError(f"{what}: expected descriptors [M,L,{VIEWS},{DESC_BYTES}] with M >= 1, got "
                         f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if not 1 <= t.shape[1] <= MAX_FIELDS:
        raise ValueError(f"{what}: 1 to {MAX_FIELDS} light fields per model, got {t.shape[1]}")
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: descriptors must be uint8, got {t.dtype}")
    _gpu(t, what)
    return t.detach().contiguous()


def _perms(perms):
    p = rotation_perms() if perms is None else np.ascontiguousarray(np.asarray(perms.cpu() if torch.is_tensor(perms) else perms))
    if p.ndim != 2 or p.shape[1] != VIEWS or not 1 <= p.shape[0] <= MAX_ROTATIONS:
        raise ValueError(f"lfd_matrix: perms must be [G,{VIEWS}] with 1 <= G <= {MAX_ROTATIONS}, got {p.shape}")
    if p.dtype.kind not in "iu" or int(p.min()) < 0 or int(p.max()) >= VIEWS:
        raise ValueError(f"lfd_matrix: every entry of perms must be an integer in [0, {VIEWS})")
    return torch.from_numpy(p.astype(np.uint8))


def lfd_matrix(x, y=None, perms=None):
    """x uint8 [Nx,L,10,48], y uint8 [Ny,L,10,48] on the GPU -> int32 [Nx,Ny]: md_lfd_matrix,
        out[i,j] = min over la, lb < L and g of sum_v SAD48(x[i,la,v], y[j,lb,perms[g,v]]),
    with perms = `rotation_perms()` unless given ([G,10], G <= 64, on the host).  Exact integers, at most 10 * 48 * 255.
    y=None or y is x: the triangular union launch -- the pairs i < j only, exactly symmetric, a zero diagonal (for a full launch the
    diagonal is zero as well when perms holds the identity).  Not differentiable."""
    xc = _models(x, "lfd_matrix")
    tri = y is None or y is x
    yc = xc if tri else _models(y, "lfd_matrix")
    if yc.device != xc.device:
        raise ValueError("lfd_matrix: both sets of descriptors need the same device")
    if yc.shape[1] != xc.shape[1]:
        raise ValueError(f"lfd_matrix: both sets need the same number of light fields, got {xc.shape[1]} and {yc.shape[1]}")
    p = _perms(perms)
    out = torch.empty((xc.shape[0], yc.shape[0]), dtype=torch.int32, device=xc.device)
    call("md_lfd_matrix", xc, yc, p, xc.shape[0], yc.shape[0], xc.shape[1], p.shape[0], 1 if tri else 0, out)
    return out


def lfd_metrics(sample_desc, ref_desc):
    """MMD / COV / 1-NNA under the light-field distance of samples [S,L,10,48] against references [R,L,10,48]: ONE triangular
    `lfd_matrix` of the concatenation, converted to float64 and handed to `metrics.mmd_cov` and `metrics.one_nna` as they are.
    Returns {"mmd_lfd", "cov_lfd", "1nna_lfd", "1nna_lfd_sample", "1nna_lfd_ref", "n_sample", "n_ref", "lfd_fields"}."""
    from .metrics import mmd_cov, one_nna
    s, r = _models(sample_desc, "lfd_metrics"), _models(ref_desc, "lfd_metrics")
    if s.device != r.device or s.shape[1] != r.shape[1]:
        raise ValueError("lfd_metrics: both sets need the same device and the same number of light fields")
    S = s.shape[0]
    d = lfd_matrix(torch.cat([s, r], dim=0)).to(torch.float64)
    mmd, cov = mmd_cov(d[:S, S:])
    acc, acc_s, acc_r = one_nna(d[:S, :S], d[:S, S:], d[S:, S:])
    return {"mmd_lfd": mmd, "cov_lfd": cov, "1nna_lfd": acc, "1nna_lfd_sample": acc_s, "1nna_lfd_ref": acc_r, "n_sample": S,
            "n_ref": r.shape[0], "lfd_fields": int(s.shape[1])}
