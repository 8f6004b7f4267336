"""Marching tetrahedra on MI355X -- host side of md_marching_tets.

Drop-in for the reference's nvdiffrec/lib/geometry/dmtet.py `DMTet.__call__` :105-163
(same signature and 6-tuple result) plus the grid -> tet-vertex gather of
nvdiffrec/eval.py:389-419 / `get_deformed` dmtet.py:293-304 and the grid-mask construction of
data/get_tet_mask.py:9-37.

Static preprocessing (once per tet grid, torch ops): the lexicographically sorted unique edge list
of ALL tets and the [T,6] tet->edge-id table.  Per call: four launches (chunked over edges / tets) for M meshes.

The vertex interpolation is differentiable as in the reference (only its topology part sits under no_grad there):
when `pos` or `sdf` requires a gradient, `verts` carries a grad_fn whose backward is md_marching_tets_bwd, one gather
launch over a static incidence list (no atomics: bit-reproducible).  `sdf_reg_loss` (dmtet.py:169-175) and the part of
`DMTetGeometry` (dmtet.py:203-304) that needs no renderer complete the fitting loop fit -> dict -> training grid.

The fixed-topology second pass (fit_dmtets.py:758-793): `FixedTopoPlan` keeps what depends on the sign of the SDF alone (faces, the
crossing edges, the CSRs, the edge neighbours) and moves the vertices with md_fixedtopo_verts / md_fixedtopo_verts_bwd, by the
contract in the header comment of csrc/fixedtopo.hip; `DMTetGeometryFixedTopo` (dmtet_fixedtopo.py:176-288) is the geometry on it.
"""
import os
import types

import numpy as np
import torch

from . import _lib
from ._csr import csr_by_row
from .hip_ops import _ptr, _stream, call

BASE_TET_EDGES = (0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3)


class TetTables:
    """Static tables of one tet grid, resident on the device."""

    def __init__(self, tets, device):
        tets = torch.as_tensor(tets).to(device=device, dtype=torch.int64)
        be = torch.tensor(BASE_TET_EDGES, dtype=torch.int64, device=device)
        e = tets[:, be].reshape(-1, 2)
        e = torch.stack([e.min(dim=1).values, e.max(dim=1).values], dim=-1)
        uniq, inv = torch.unique(e, dim=0, return_inverse=True)  # rows sorted lexicographically
        self.n_tets, self.n_edges = tets.shape[0], uniq.shape[0]
        self.tets = tets.to(torch.int32).contiguous()
        self.edges = uniq.to(torch.int32).contiguous()
        self.tet_edges = inv.reshape(-1, 6).to(torch.int32).contiguous()
        self.tets64 = tets
        self._incidence, self._all_edges = {}, None

    def incidence(self, n_verts):
        """(inc_ptr int32 [N+1], inc int32 [2E]) of the edge table, built at the first call that needs a gradient."""
        if n_verts not in self._incidence:
            self._incidence = {n_verts: build_incidence(self.edges, n_verts)}
        return self._incidence[n_verts]

    @property
    def all_edges(self):
        """The reference's `DMTetGeometry.all_edges` (int64 [E,2]); `sdf_reg_loss` recognises it and uses these tables."""
        if self._all_edges is None:
            self._all_edges = self.edges.long()
            self._all_edges._md_tables = self
        return self._all_edges


def build_incidence(edges, n_verts):
    """CSR over grid vertices of an edge table [E,2]: inc_ptr int32 [N+1], inc int32 [2E] with inc = 2 * edge id + (0 if the
    vertex is the edge's first endpoint, 1 if its second), ascending edge id inside a vertex.  Every edge appears twice.
    Checks once (on the host) that no edge names a vertex >= n_verts: the kernels index with these tables unchecked."""
    e = edges.long()
    E = e.shape[0]
    if E == 0 or int(e.min()) < 0 or int(e.max()) >= n_verts:
        raise ValueError(f"edge table names vertices outside [0, {n_verts})")
    ids = torch.arange(E, dtype=torch.int64, device=e.device)
    vert = torch.cat([e[:, 0], e[:, 1]])
    code = torch.cat([2 * ids, 2 * ids + 1])
    order = torch.argsort(vert * (2 * E) + code)          # unique keys: by vertex, then by edge id
    inc = code[order].to(torch.int32).contiguous()
    inc_ptr = torch.zeros(n_verts + 1, dtype=torch.int64, device=e.device)
    inc_ptr[1:] = torch.cumsum(torch.bincount(vert, minlength=n_verts), 0)
    return inc_ptr.to(torch.int32).contiguous(), inc


class MeshCounts:
    """Per-mesh (vertices, faces, 1-triangle tets, 2-triangle tets) of one md_marching_tets call: int32 [M, 4], copied to a pinned
    host buffer ASYNCHRONOUSLY on the launch stream; the first host read waits for that copy's event.  Behaves like the numpy
    array (indexing, np.asarray, .sum through it)."""

    def __init__(self, dev_counts):
        self.device_counts = dev_counts                       # consumers on the GPU can read the sizes without any host sync
        self._host = torch.empty(dev_counts.shape, dtype=torch.int32, pin_memory=True)
        self._host.copy_(dev_counts, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()
        self._np = None

    def numpy(self):
        if self._np is None:
            self._event.synchronize()
            self._np = self._host.numpy()
        return self._np

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype)

    def __getitem__(self, k):
        return self.numpy()[k]

    def __len__(self):
        return self._host.shape[0]

    @property
    def shape(self):
        return tuple(self._host.shape)


class MeshBatch:
    """The M meshes of one md_marching_tets call as a lazy sequence of (verts [V,3], faces [F,3] int64, face_tet [F]) views into
    the call's output buffers (allocated at their static bounds V <= E, F <= 2T): the trimming -- which needs the counts on the
    host -- happens at the first access, not inside the call, so a caller that queues more GPU work does not stall on it."""

    def __init__(self, verts, faces, face_tet, counts):
        self.verts, self.faces, self.face_tet, self.counts = verts, faces, face_tet, counts

    def __len__(self):
        return self.verts.shape[0]

    def __getitem__(self, m):
        if isinstance(m, slice):
            return [self[i] for i in range(*m.indices(len(self)))]
        if m < 0:
            m += len(self)
        if not 0 <= m < len(self):
            raise IndexError(m)
        c = self.counts.numpy()
        nv, nf = int(c[m, 0]), int(c[m, 1])
        return self.verts[m, :nv], self.faces[m, :nf], self.face_tet[m, :nf]

    def __iter__(self):
        return (self[m] for m in range(len(self)))


_MT_WORKSPACE = {}


def _mt_workspace(nbytes, device):
    """The call's scratch (edge -> vertex ids, chunk offsets) is dead when its last kernel ends: one buffer per (device, stream),
    grown to the largest request -- launches on a stream are ordered, so consecutive calls can share it."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _MT_WORKSPACE.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _MT_WORKSPACE[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return buf


def release_workspace():
    """Drop the per-stream scratch buffers of md_marching_tets (the next call allocates again)."""
    _MT_WORKSPACE.clear()


def _mt_launch(lib, pos, sdf, tables, ws, ws_bytes):
    M, N = sdf.shape
    E, T = tables.n_edges, tables.n_tets
    dev = pos.device
    verts = torch.empty((M, E, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((M, 2 * T, 4), dtype=torch.int64, device=dev)     # [..., :3] faces, then M * 2T face -> tet ids behind them
    face_tet = faces.view(-1)[M * 2 * T * 3:].view(M, 2 * T)
    counts = torch.empty((M, 4), dtype=torch.int32, device=dev)
    _lib.check(lib.md_marching_tets(_ptr(pos), _ptr(sdf), _ptr(tables.tets), _ptr(tables.edges),
                                    _ptr(tables.tet_edges), M, N, E, T, _ptr(verts), _ptr(faces),
                                    _ptr(face_tet), _ptr(counts), _ptr(ws), ws_bytes, _stream()),
               "md_marching_tets")
    return verts, faces, counts


class _MarchingTetsFn(torch.autograd.Function):
    """md_marching_tets with md_marching_tets_bwd as the backward of `verts` w.r.t. (pos, sdf).  The call owns its workspace
    (the per-stream one is overwritten by the next call) and keeps the edge -> vertex id table and the counts."""

    @staticmethod
    def forward(ctx, pos, sdf, tables):
        lib = _lib.load()
        M, N = sdf.shape
        ws_bytes = lib.md_marching_tets_workspace_bytes(M, tables.n_edges, tables.n_tets)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
        verts, faces, counts = _mt_launch(lib, pos, sdf, tables, ws, ws_bytes)
        ctx.tables = tables
        ctx.save_for_backward(pos, sdf, ws, counts)
        ctx.mark_non_differentiable(faces, counts)
        return verts, faces, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_verts, _gf, _gc):
        pos, sdf, ws, counts = ctx.saved_tensors
        tb = ctx.tables
        M, N = sdf.shape
        inc_ptr, inc = tb.incidence(N)
        g = grad_verts.to(torch.float32).contiguous()
        dpos, dsdf = torch.empty_like(pos), torch.empty_like(sdf)
        call("md_marching_tets_bwd", pos, sdf, tb.edges, ws, counts, g, inc_ptr, inc, M, N, tb.n_edges, dpos, dsdf)
        return (dpos if ctx.needs_input_grad[0] else None), (dsdf if ctx.needs_input_grad[1] else None), None


def marching_tets_batch(pos, sdf, tables):
    """pos [M,N,3] f32, sdf [M,N] f32 on the GPU -> (MeshBatch, MeshCounts): meshes[m] = (verts [V,3], faces [F,3] int64,
    face_tet [F]), counts[m] = (V, F, 1-triangle tets, 2-triangle tets).  No host synchronisation inside the call: the counts
    travel to a pinned buffer behind the kernels and are awaited at the first read.
    When grad mode is on and `pos` or `sdf` requires a gradient, the vertices carry a grad_fn (first derivatives only)."""
    lib = _lib.load()
    if not pos.is_cuda:
        raise _lib.MeshDiffusionHipError("marching tets runs on the GPU only (no CPU fallback)")
    pos = pos.to(torch.float32).contiguous()
    sdf = sdf.to(torch.float32).contiguous()
    M, N = sdf.shape
    E, T = tables.n_edges, tables.n_tets
    if torch.is_grad_enabled() and (pos.requires_grad or sdf.requires_grad):
        verts, faces, counts = _MarchingTetsFn.apply(pos, sdf, tables)
    else:
        ws_bytes = lib.md_marching_tets_workspace_bytes(M, E, T)
        verts, faces, counts = _mt_launch(lib, pos, sdf, tables, _mt_workspace(ws_bytes, pos.device), ws_bytes)
    face_tet = faces.view(-1)[M * 2 * T * 3:].view(M, 2 * T)
    faces = faces.view(-1)[:M * 2 * T * 3].view(M, 2 * T, 3)
    cnt = MeshCounts(counts)
    return MeshBatch(verts, faces, face_tet, cnt), cnt


def _map_uv(face_tet, n1, num_tets, device):
    """Per-tet texture atlas (dmtet.py:70-99): face_gidx = 2*tet (+1 for a tet's second triangle)."""
    max_idx = num_tets * 2
    Nn = int(np.ceil(np.sqrt((max_idx + 1) // 2)))
    lin = torch.linspace(0, 1 - (1 / Nn), Nn, dtype=torch.float32, device=device)
    tex_y, tex_x = torch.meshgrid(lin, lin, indexing="ij")
    pad = 0.9 / Nn
    uvs = torch.stack([tex_x, tex_y, tex_x + pad, tex_y, tex_x + pad, tex_y + pad, tex_x, tex_y + pad],
                      dim=-1).view(-1, 2)
    F = face_tet.shape[0]
    tri_idx = torch.zeros(F, dtype=torch.int64, device=device)
    if F > n1:
        tri_idx[n1:] = torch.arange(F - n1, device=device) % 2
    tet_idx = face_tet  # (face_gidx // 2); _idx(t, N) = (t // N) * N + t % N = t
    uv_idx = torch.stack((tet_idx * 4, tet_idx * 4 + tri_idx + 1, tet_idx * 4 + tri_idx + 2), dim=-1).view(-1, 3)
    return uvs, uv_idx


class DMTet:
    """`DMTet()(pos_nx3, sdf_n, tet_fx4) -> (verts, faces, uvs, uv_idx, face_to_valid_tet, valid_vert_idx)`."""

    def __init__(self):
        self._tables = {}

    def tables_for(self, tet_fx4):
        key = (tet_fx4.data_ptr(), tuple(tet_fx4.shape), str(tet_fx4.device), tet_fx4._version)
        if key not in self._tables:
            self._tables = {key: TetTables(tet_fx4, tet_fx4.device)}
        return self._tables[key]

    def __call__(self, pos_nx3, sdf_n, tet_fx4):
        with torch.no_grad():
            tb = self.tables_for(tet_fx4)
        # as in the reference, only the topology is constant: verts is differentiable w.r.t. pos_nx3 and sdf_n
        meshes, cnt = marching_tets_batch(pos_nx3[None], sdf_n[None], tb)
        verts, faces, face_tet = meshes[0]
        with torch.no_grad():
            uvs, uv_idx = _map_uv(face_tet, int(cnt[0, 2]), tb.n_tets, verts.device)
            tets_used = torch.unique(face_tet)
            valid_vert_idx = tb.tets64[tets_used].long().unique()
            return verts, faces, uvs, uv_idx, face_tet.long(), valid_vert_idx


# ---- cubic grid <-> tet grid ---------------------------------------------------------------------
def tet_vertices_to_grid_index(vertices):
    """eval.py:389-398 / evaler.py:187-195: tet-vertex positions -> integer grid coordinates."""
    v = torch.as_tensor(vertices)
    uniq = v[:].unique()
    dx = uniq[1] - uniq[0]
    return torch.round((v - v.min()) / dx).long()


def grid_mask_from_tets(vertices, R):
    """data/get_tet_mask.py:9-37: 1 where a tet-grid vertex lives, else 0.  float32 [R,R,R]."""
    idx = tet_vertices_to_grid_index(vertices)
    m = torch.zeros(R, R, R)
    m[idx[:, 0], idx[:, 1], idx[:, 2]] = 1.0
    return m


class GridMesher:
    """`.npy` grids [M,4,R,R,R] -> meshes, the eval.py:400-431 path without the renderer.  With `grids` that require a gradient the
    vertices are differentiable w.r.t. the deformation channels (zero outside [-1, 1], where the clip is flat); channel 0 goes
    through `sign` and receives zero, as in eval.py:412-419."""

    def __init__(self, tet_vertices, tet_indices, R, mesh_scale=2.1, deform_scale=2.0, device="cuda"):
        self.R, self.deform_scale = R, deform_scale
        dev = torch.device(device)
        v = torch.as_tensor(tet_vertices, dtype=torch.float32)
        self.idx = tet_vertices_to_grid_index(v).to(dev)
        self.verts = (v * mesh_scale).to(dev)            # dmtet.py:219
        self.tables = TetTables(torch.as_tensor(tet_indices), dev)

    def inputs(self, grids):
        g = torch.as_tensor(grids).to(self.verts.device, torch.float32)
        i0, i1, i2 = self.idx[:, 0], self.idx[:, 1], self.idx[:, 2]
        sdf = torch.sign(g[:, 0][:, i0, i1, i2])                              # [M,N]
        deform = g[:, 1:][:, :, i0, i1, i2].transpose(1, 2).clip(-1.0, 1.0)     # [M,N,3]
        pos = self.verts[None] + 2 / (self.R * 2) * deform * self.deform_scale  # dmtet.py:303
        return pos.contiguous(), sdf.contiguous()

    def __call__(self, grids):
        pos, sdf = self.inputs(grids)
        meshes, _ = marching_tets_batch(pos, sdf, self.tables)
        return meshes


# ---- regulariser and geometry of the fitting loop -------------------------------------------------
class _EdgeTables:
    """Edge table + incidence list of an arbitrary [E,2] edge tensor handed to sdf_reg_loss."""

    def __init__(self, edges):
        self.edges = edges.to(torch.int32).contiguous()
        self.n_edges = self.edges.shape[0]
        self._incidence = {}

    incidence = TetTables.incidence


_EDGE_TABLES = {}


def _edge_tables_for(all_edges):
    if isinstance(all_edges, (TetTables, _EdgeTables)):
        return all_edges
    tb = getattr(all_edges, "_md_tables", None)
    if tb is not None:
        return tb
    key = (all_edges.data_ptr(), tuple(all_edges.shape), str(all_edges.device), all_edges._version)
    if key not in _EDGE_TABLES:
        _EDGE_TABLES.clear()
        _EDGE_TABLES[key] = _EdgeTables(all_edges.reshape(-1, 2))
    return _EDGE_TABLES[key]


class _SdfRegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sdf, tables):
        dev = sdf.device
        ws = torch.empty(_lib.SDF_REG_WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        call("md_sdf_reg_loss", sdf, tables.edges, sdf.shape[0], tables.n_edges, ws, loss, count)
        ctx.tables = tables
        ctx.save_for_backward(sdf, count)
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        sdf, count = ctx.saved_tensors
        tb = ctx.tables
        inc_ptr, inc = tb.incidence(sdf.shape[0])
        g = grad_out.to(torch.float32).reshape(1).contiguous()
        dsdf = torch.empty_like(sdf)
        call("md_sdf_reg_loss_bwd", sdf, tb.edges, inc_ptr, inc, count, g, sdf.shape[0], tb.n_edges, dsdf)
        return dsdf, None


def sdf_reg_loss(sdf, all_edges):
    """The reference's regulariser (dmtet.py:169-175), same signature: over the edges whose endpoints differ in `torch.sign`,
    mean bce_with_logits(s0, [s1 > 0]) + mean bce_with_logits(s1, [s0 > 0]) -- md_sdf_reg_loss, differentiable w.r.t. sdf.
    `all_edges`: `TetTables.all_edges` / `DMTetGeometry.all_edges` (their tables are reused), a `TetTables`, or any [E,2] edge
    tensor on the GPU.  An empty mask returns nan with a zero gradient: the reference's mean of an empty tensor, kept."""
    if not sdf.is_cuda:
        raise _lib.MeshDiffusionHipError("sdf_reg_loss runs on the GPU only (no CPU fallback)")
    tb = _edge_tables_for(all_edges)
    if tb.edges.device != sdf.device:
        raise _lib.MeshDiffusionHipError("sdf_reg_loss: the edge table and sdf are on different devices")
    if getattr(tb, "_vertex_range", None) is None:                  # once per table: the kernel indexes sdf unchecked
        tb._vertex_range = (int(tb.edges.min()), int(tb.edges.max()))
    if tb._vertex_range[0] < 0 or tb._vertex_range[1] >= sdf.numel():
        raise ValueError(f"sdf_reg_loss: the edge table names vertices outside [0, {sdf.numel()})")
    return _SdfRegLossFn.apply(sdf.to(torch.float32).reshape(-1).contiguous(), tb)


class DMTetGeometry(torch.nn.Module):
    """The part of the reference's DMTetGeometry (dmtet.py:203-304) that needs no renderer: the `sdf` / `deform` parameters
    of one tet grid with the reference's initialisation, the edge list of the regulariser, the deformed vertices and the
    differentiable mesh.  The tet grid is read from `{root}/data/tets/{grid_res}_tets_cropped.npz` as in the reference, or
    passed as `tets=(vertices, indices)`.  No EMA copies, no sign buffer, no material."""

    def __init__(self, grid_res, scale, FLAGS=None, root="./", grid_to_tet=None, deform_scale=1.0, tets=None, device="cuda",
                 **kwargs):
        super().__init__()
        self.FLAGS, self.grid_res, self.deform_scale, self.grid_to_tet = FLAGS, grid_res, deform_scale, grid_to_tet
        self.marching_tets = DMTet()
        self.tanh = False
        if tets is None:
            t = np.load(os.path.join(root, "data/tets/{}_tets_cropped.npz".format(grid_res)))
            tets = (t["vertices"], t["indices"])
        self.tet_vertices = torch.as_tensor(np.asarray(tets[0]), dtype=torch.float32)      # unscaled, for the grid index
        self.verts = self.tet_vertices.to(device) * scale
        self.indices = torch.as_tensor(np.asarray(tets[1]), dtype=torch.long).to(device)
        self.generate_edges()
        sdf = torch.rand_like(self.verts[:, 0]).clamp(-1.0, 1.0) - 0.1                       # dmtet.py:224
        self.sdf = torch.nn.Parameter(sdf.clone().detach(), requires_grad=True)
        self.deform = torch.nn.Parameter(torch.zeros_like(self.verts), requires_grad=True)

    def generate_edges(self):
        with torch.no_grad():
            self.all_edges = self.marching_tets.tables_for(self.indices).all_edges

    def getAABB(self):
        return torch.min(self.verts, dim=0).values, torch.max(self.verts, dim=0).values

    def getVertNNDist(self):
        """Squared distance of every deformed grid vertex to its nearest OTHER vertex (dmtet.py:249-251, the reference's
        knn_points(v, v, K=2).dists[0, :, -1]): md_nn_sided with skip_same_index.  Detached, float32 [N]."""
        from .pointcloud import sided_distance
        v_deformed = (self.verts + 2 / (self.grid_res * 2) * torch.tanh(self.deform)).unsqueeze(0)
        return sided_distance(v_deformed, v_deformed, skip_same_index=True)[0][0]

    def getTetCenters(self):
        return self.get_deformed()[self.indices].mean(dim=1)

    def getValidTetIdx(self):
        return self.marching_tets(self.get_deformed(), self.sdf, self.indices)[4].long()

    def getValidVertsIdx(self):
        return self.indices[self.getValidTetIdx()].unique()

    def clamp_deform(self):
        if not self.tanh:
            self.deform.data[:] = self.deform.data.clamp(-0.99, 0.99)
            self.sdf.data[:] = self.sdf.data.clamp(-1.0, 1.0)

    def get_deformed(self, no_grad=False):
        deform = self.deform.detach() if no_grad else self.deform
        if self.tanh:
            return self.verts + 2 / (self.grid_res * 2) * torch.tanh(deform) * self.deform_scale
        return self.verts + 2 / (self.grid_res * 2) * deform * self.deform_scale

    def getMesh(self, material=None, normals_grad=False):
        """Named like the reference's Mesh: v_pos (differentiable), t_pos_idx, v_tex, t_tex_idx, v_nrm / t_nrm_idx (smooth
        normals, detached; with normals_grad=True from `vertex_normals` and attached to the graph), valid_vert_idx."""
        verts, faces, uvs, uv_idx, _tet_gidx, valid_vert_idx = self.marching_tets(self.get_deformed(), self.sdf, self.indices)
        if normals_grad and verts.shape[0] > 0:
            v_nrm = vertex_normals(verts, faces)[0]
        else:
            v_nrm = auto_normals(verts.detach(), faces)[0] if verts.shape[0] > 0 else torch.zeros_like(verts)
        return types.SimpleNamespace(v_pos=verts, t_pos_idx=faces, v_tex=uvs, t_tex_idx=uv_idx, v_nrm=v_nrm, t_nrm_idx=faces,
                                     material=material, valid_vert_idx=valid_vert_idx)

    def init_with_gt_surface(self, gt_verts, surface_faces, campos):
        """dmtet_singleview.py:421-435: sdf = 1.0 on the camera's side of the nearest visible face (`singleview.init_with_gt_surface`)."""
        from .singleview import init_with_gt_surface
        return init_with_gt_surface(self, gt_verts, surface_faces, campos)

    def state_to_dict(self):
        """The `{'sdf', 'deform'}` dict fit_dmtets.py saves and mesh_export.dicts_to_grids reads."""
        return {"sdf": self.sdf.detach().cpu(), "deform": self.deform.detach().cpu()}


# ---- the fixed-topology second pass -------------------------------------------------------------------------------------------------
class _FixedTopoVertsFn(torch.autograd.Function):
    """md_fixedtopo_verts with md_fixedtopo_verts_bwd as the backward of `verts` w.r.t. pos; the frozen SDF gets no gradient."""

    @staticmethod
    def forward(ctx, pos, sdf, plan):
        verts = torch.empty((plan.n_mesh_verts, 3), dtype=torch.float32, device=pos.device)
        call("md_fixedtopo_verts", pos, sdf, plan.edge, pos.shape[0], plan.n_mesh_verts, verts)
        ctx.plan = plan
        ctx.save_for_backward(sdf)
        return verts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        sdf, = ctx.saved_tensors
        plan = ctx.plan
        g = g.to(torch.float32).contiguous()
        dpos = torch.empty((sdf.shape[0], 3), dtype=torch.float32, device=g.device)
        call("md_fixedtopo_verts_bwd", g, sdf, plan.edge, plan.inc_ptr, plan.inc, sdf.shape[0], plan.n_mesh_verts, dpos)
        return dpos, None, None


class FixedTopoPlan:
    """Everything about the mesh of one tet grid that depends on the SIGN of the SDF alone, by the fixed-topology contract in the
    header comment of csrc/fixedtopo.hip: built once from one run of the existing marching tetrahedra (under no_grad), then
    `verts(pos, sdf)` moves the vertices with one launch and no topology search, no counts and no device-to-host read.
      faces int64 [F,3], uvs, uv_idx, face_tet int64 [F], valid_vert_idx    what `DMTet()` returns for this sign
      edge int32 [Vm,2]                       the grid endpoints of each mesh vertex: the crossing edges in ascending edge id
      inc_ptr int32 [N+1], inc int32 [2 Vm]   grid-vertex CSR of the codes 2 * mesh vertex + endpoint (`build_incidence(edge, N)`)
      corner_csr                              `face_corner_csr(faces, Vm)`, for `vertex_normals(csr=)` and the Laplacian
      neighbours int32 [F,3]                  `render.edge_neighbours(faces, Vm)`, for `render_depth / render_buffers(neighbours=)`
    tables: the grid's `TetTables`; pos float32 [N,3], sdf float32 [N] on the GPU (only the sign of sdf matters)."""

    def __init__(self, tables, pos, sdf):
        from .render import edge_neighbours
        if not (torch.is_tensor(pos) and pos.is_cuda and torch.is_tensor(sdf) and sdf.is_cuda):
            raise _lib.MeshDiffusionHipError("FixedTopoPlan runs on the GPU only (no CPU fallback)")
        if pos.dim() != 2 or pos.shape[-1] != 3 or sdf.dim() != 1 or sdf.shape[0] != pos.shape[0]:
            raise ValueError(f"FixedTopoPlan: expected pos [N,3] and sdf [N], got {tuple(pos.shape)} and {tuple(sdf.shape)}")
        with torch.no_grad():
            pos = pos.detach().to(torch.float32).contiguous()
            sdf = sdf.detach().to(torch.float32).contiguous()
            meshes, cnt = marching_tets_batch(pos[None], sdf[None], tables)
            verts, faces, face_tet = meshes[0]
            if verts.shape[0] == 0 or faces.shape[0] == 0:
                raise _lib.MeshDiffusionHipError("FixedTopoPlan: the sign field has no surface")
            self.tables, self.n_grid_verts, self.n_mesh_verts = tables, pos.shape[0], verts.shape[0]
            self.faces = faces.clone()                                         # not views into the call's 2 T rows
            self.face_tet = face_tet.long().clone()
            self.uvs, self.uv_idx = _map_uv(face_tet, int(cnt[0, 2]), tables.n_tets, pos.device)
            self.valid_vert_idx = tables.tets64[torch.unique(face_tet)].long().unique()
            e = tables.edges.long()
            pos_sign = sdf > 0
            self.edge = tables.edges[pos_sign[e[:, 0]] != pos_sign[e[:, 1]]].contiguous()          # ascending edge id
            if self.edge.shape[0] != self.n_mesh_verts:
                raise _lib.MeshDiffusionHipError("FixedTopoPlan: the crossing edges do not match the marching-tets vertices")
            self.inc_ptr, self.inc = build_incidence(self.edge, self.n_grid_verts)
            self.corner_csr = face_corner_csr(self.faces, self.n_mesh_verts)
            self.neighbours = edge_neighbours(self.faces, self.n_mesh_verts)
            self.initial_verts = verts.clone()

    def verts(self, pos, sdf):
        """verts float32 [Vm,3] of pos [N,3], sdf [N] whose signs are the plan's: bit-equal to `marching_tets_batch` on the same
        inputs; differentiable w.r.t. pos (bit-equal to the existing backward), no gradient for sdf."""
        if not (pos.is_cuda and sdf.is_cuda):
            raise _lib.MeshDiffusionHipError("FixedTopoPlan.verts runs on the GPU only (no CPU fallback)")
        if tuple(pos.shape) != (self.n_grid_verts, 3) or tuple(sdf.shape) != (self.n_grid_verts,):
            raise ValueError(f"FixedTopoPlan.verts: expected pos [{self.n_grid_verts},3] and sdf [{self.n_grid_verts}], got "
                             f"{tuple(pos.shape)} and {tuple(sdf.shape)}")
        return _FixedTopoVertsFn.apply(pos.to(torch.float32).contiguous(), sdf.detach().to(torch.float32).contiguous(), self)


def fixed_sign(sdf):
    """The frozen sign of pass 2 (dmtet_fixedtopo.py:194-195): sign(sdf + 1e-8) with zeros set to +1.  Plain torch."""
    s = torch.sign(sdf.detach() + 1e-8).float()
    s[s == 0] = 1.0
    return s


class DMTetGeometryFixedTopo(torch.nn.Module):
    """The reference's DMTetGeometryFixedTopo (dmtet_fixedtopo.py:176-288) without its renderer: pass 2 of the fit.  The sign of
    `dmt_geometry.sdf` is frozen (`sdf_sign`, zeros -> +1), `sdf_abs` = 1 is frozen too, and `deform` -- taken over from pass 1;
    the caller rescales it by first_stage_deform / second_stage_deform as fit_dmtets.py:770 does -- is the only trainable tensor.
    The `FixedTopoPlan` is built at construction (`plan`), so `getMesh` runs no topology search; assigning `geo.sdf_sign = s`
    rebuilds it.  tets=(vertices, indices) or None to take the grid of `dmt_geometry`.  No EMA copies, no material."""

    def __init__(self, dmt_geometry, grid_res, scale, FLAGS=None, deform_scale=1.0, tets=None, **kwargs):
        super().__init__()
        self.FLAGS, self.grid_res, self.scale, self.deform_scale, self.tanh = FLAGS, grid_res, scale, deform_scale, False
        dev = dmt_geometry.sdf.device
        if not dev.type == "cuda":
            raise _lib.MeshDiffusionHipError("DMTetGeometryFixedTopo runs on the GPU only (no CPU fallback)")
        self.marching_tets = DMTet()
        if tets is None:
            self.tet_vertices, self.indices = dmt_geometry.tet_vertices, dmt_geometry.indices.to(dev)
        else:
            self.tet_vertices = torch.as_tensor(np.asarray(tets[0]), dtype=torch.float32)
            self.indices = torch.as_tensor(np.asarray(tets[1]), dtype=torch.long).to(dev)
        self.verts = self.tet_vertices.to(dev) * scale
        self.generate_edges()
        self._parameters["sdf_sign"] = torch.nn.Parameter(fixed_sign(dmt_geometry.sdf.data), requires_grad=False)
        self.sdf_abs = torch.nn.Parameter(torch.ones_like(dmt_geometry.sdf.data), requires_grad=False)
        self.deform = torch.nn.Parameter(dmt_geometry.deform.data.clone(), requires_grad=True)
        self._build_plan()

    def __setattr__(self, name, value):
        if name == "sdf_sign" and "sdf_sign" in self._parameters:               # a new sign is a new topology
            with torch.no_grad():
                self._parameters["sdf_sign"].copy_(fixed_sign(torch.as_tensor(value).to(self._parameters["sdf_sign"].device)))
            self._build_plan()
            return
        super().__setattr__(name, value)

    def _build_plan(self):
        with torch.no_grad():
            self._sdf = (self.sdf_sign * self.sdf_abs.abs()).contiguous()
            self.plan = FixedTopoPlan(self.marching_tets.tables_for(self.indices), self.get_deformed(), self._sdf)
        self.initial_guess_v_pos = self.plan.initial_verts

    generate_edges = DMTetGeometry.generate_edges
    getAABB = DMTetGeometry.getAABB
    getTetCenters = DMTetGeometry.getTetCenters
    get_deformed = DMTetGeometry.get_deformed

    def set_init_v_pos(self):
        """The vertices the Laplacian measures the displacement from (dmtet_fixedtopo.py:207-211): those of the current deform."""
        with torch.no_grad():
            self.initial_guess_v_pos = self.plan.verts(self.get_deformed(), self._sdf)

    def getValidTetIdx(self):
        return self.plan.face_tet

    def getValidVertsIdx(self):
        return self.plan.valid_vert_idx

    def clamp_deform(self):
        if not self.tanh:
            self.deform.data[:] = self.deform.data.clamp(-0.99, 0.99)

    def getMesh(self, material=None, normals_grad=False):
        """The namespace of `DMTetGeometry.getMesh`, through the plan: one launch for the vertices, the plan's faces and uvs."""
        plan = self.plan
        verts = plan.verts(self.get_deformed(), self._sdf)
        if normals_grad:
            v_nrm = vertex_normals(verts, plan.faces, csr=plan.corner_csr)[0]
        else:
            v_nrm = auto_normals(verts.detach(), plan.faces)[0]
        return types.SimpleNamespace(v_pos=verts, t_pos_idx=plan.faces, v_tex=plan.uvs, t_tex_idx=plan.uv_idx, v_nrm=v_nrm,
                                     t_nrm_idx=plan.faces, material=material, valid_vert_idx=plan.valid_vert_idx)

    def state_to_dict(self):
        """The dict fit_dmtets.py:784-793 saves under tets/: the sign, the deformation masked to the vertices of the surface
        tets, and the unmasked deformation."""
        vert_mask = torch.zeros_like(self.sdf_sign).long().view(-1, 1)
        vert_mask[self.getValidVertsIdx()] = 1
        return {"sdf": self.sdf_sign.detach().cpu(), "deform": (self.deform.detach() * vert_mask).cpu(),
                "deform_unmasked": self.deform.detach().cpu()}


def auto_normals(verts, faces):
    """Smooth vertex normals of a mesh (nvdiffrec/lib/render/mesh.py:200-229, the call at nvdiffrec/eval.py:422 on the
    marching-tets output): returns (v_nrm float32 [V,3], f_nrm float32 [F,3] unnormalised) -- md_vertex_normals."""
    if not verts.is_cuda:
        raise _lib.MeshDiffusionHipError("auto_normals runs on the GPU only")
    v = verts.to(torch.float32).contiguous()
    f = faces.to(torch.int64).contiguous()
    v_nrm = torch.empty_like(v)
    f_nrm = torch.empty((f.shape[0], 3), dtype=torch.float32, device=v.device)
    call("md_vertex_normals", v, f, v.shape[0], f.shape[0], v_nrm, f_nrm)
    return v_nrm, f_nrm


class _VertexNormalsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces, ptr, order):
        V, F = verts.shape[0], faces.shape[0]
        v_nrm = torch.empty_like(verts)
        f_nrm = torch.empty((F, 3), dtype=torch.float32, device=verts.device)
        v_len = torch.empty(V, dtype=torch.float32, device=verts.device)
        call("md_vertex_normals_det", verts, faces, ptr, order, V, F, v_nrm, f_nrm, v_len)
        ctx.save_for_backward(verts, faces, ptr, order, v_nrm, v_len)
        return v_nrm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        verts, faces, ptr, order, v_nrm, v_len = ctx.saved_tensors
        V, F = verts.shape[0], faces.shape[0]
        g = g.to(torch.float32).contiguous()
        face_grad = torch.empty((F, 3, 3), dtype=torch.float32, device=verts.device)
        dverts = torch.empty_like(verts)
        call("md_vertex_normals_bwd", verts, faces, ptr, order, v_nrm, v_len, g, V, F, face_grad, dverts)
        return dverts, None, None, None


def face_corner_csr(faces, n_verts):
    """(ptr int32 [V+1], order int32 [3F]) of the corner codes 3 f + k sorted stably by the vertex they name: the CSR of
    `vertex_normals` and `render.laplace_regularizer_const`.  faces int64 [F,3] with every index in [0, V), not checked here."""
    return csr_by_row(faces.reshape(-1), n_verts)


def _check_corner_csr(csr, n_verts, n_faces, device, what):
    ptr, order = csr
    if tuple(ptr.shape) != (n_verts + 1,) or tuple(order.shape) != (3 * n_faces,):
        raise ValueError(f"{what}: expected a face-corner CSR of shapes [{n_verts + 1}] and [{3 * n_faces}], got "
                         f"{tuple(ptr.shape)} and {tuple(order.shape)}")
    return (ptr.to(device=device, dtype=torch.int32).contiguous(), order.to(device=device, dtype=torch.int32).contiguous())


def vertex_normals(verts, faces, csr=None):
    """Smooth vertex normals under autograd, by the interpolation contract in the header comment of csrc/interp.hip (mesh.py:
    200-229): verts float32 [V,3], faces [F,3] -> (v_nrm float32 [V,3], f_nrm float32 [F,3] unnormalised).  fn_f = cross(v1 - v0,
    v2 - v0); a vertex's normal sums the fn of the corners that name it in ascending order of 3 f + k, a gather over the static
    face-corner CSR, so two runs agree bit for bit (the atomic `auto_normals` cannot promise that); a sum with s . s <= 1e-20, a
    vertex no face names included, becomes (0, 0, 1) with a zero gradient.  v_nrm is differentiable w.r.t. verts through
    md_vertex_normals_bwd, f_nrm through plain torch.
    csr: the `face_corner_csr(faces, V)` of a mesh whose faces do not change (`FixedTopoPlan.corner_csr`); None builds it, and
    checks the range of `faces`, as every call did before the keyword existed.  The bits are the same either way."""
    if not verts.is_cuda:
        raise _lib.MeshDiffusionHipError("vertex_normals runs on the GPU only (no CPU fallback)")
    if verts.dim() != 2 or verts.shape[-1] != 3 or verts.shape[0] < 1 or faces.dim() != 2 or faces.shape[-1] != 3:
        raise ValueError(f"vertex_normals: expected verts [V,3] and faces [F,3], got {tuple(verts.shape)} and {tuple(faces.shape)}")
    v = verts.to(torch.float32).contiguous()
    f = faces.to(device=v.device, dtype=torch.int64).contiguous()
    V, F = v.shape[0], f.shape[0]
    if F >= 2 ** 24:
        raise _lib.MeshDiffusionHipError("vertex_normals takes fewer than 2^24 faces (MD_ERR_UNSUPPORTED)")
    if F == 0:
        up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32, device=v.device)
        return up.expand(V, 3).contiguous(), torch.zeros((0, 3), dtype=torch.float32, device=v.device)
    if csr is None:
        lo, hi = torch.aminmax(f)
        if int(lo) < 0 or int(hi) >= V:
            raise ValueError(f"faces name vertices outside [0, {V})")
        ptr, order = face_corner_csr(f, V)
    else:
        ptr, order = _check_corner_csr(csr, V, F, v.device, "vertex_normals")
    v_nrm = _VertexNormalsFn.apply(v, f, ptr, order)
    f_nrm = torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return v_nrm, f_nrm
