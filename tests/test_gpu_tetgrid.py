"""The tet-grid kernels (md_marching_tets and its backward, the SDF regulariser and its backward, md_fixedtopo_verts and its backward)
and `GridMesher` on the synthetic grids of tests/tetgrid_cases.py: one tet, chunk edges of 1023 / 1024 / 1025 edges or tets,
255 / 256 / 257 grid vertices, a vertex with 3002 incident edges, vertices no tet names, and a 56^3 lattice whose 1229 edge
chunks and 1029 tet chunks take the second pass of the chunk scan.  tests/test_cpu_tetgrid_cases.py proves what each case owns.

Forward: bit for bit against the numpy oracle (the reference's run-time sort-and-unique algorithm) on the same fp32 inputs, and, on
the small cases, against the hashes of the unmodified reference in tests/golden/tetgrid.npz.
Gradients and regulariser: float64 restatement (tests/dmtet_grad_cases.py).  Bar = 4 x the rel-L2 distance of the SAME
restatement run in fp32 on the CPU on the same inputs from float64 (the convention of test_gpu_dmtet_grad.py, the unit computed
here and not read from a fixture), floor 2^-24: an fp32 output cannot be asked to be closer than one rounding.  Every test
prints the kernel's figure, the unit and the ratio to the bar before it asserts.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

import dmtet_grad_cases as dg
import tetgrid_cases as tc
from conftest import GOLD
from oracle import dmtet_oracle

pytestmark = pytest.mark.gpu
BAR = 4.0
FLOOR = 2.0 ** -24
REG_CASES = ("one-tet", "E1024", "star", "two-pass")
_DEV = {}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _dev(name):
    """Per case, once per module: pos and tets on the GPU, one `DMTet` (so its tables are built once), the tables, and the
    float64 restatement's edge list on the CPU."""
    if name not in _DEV:
        from meshdiffusion_amd.dmtet import DMTet
        c = tc.case(name)
        dm = DMTet()
        tets = torch.from_numpy(c.tets).long().cuda()
        tb = dm.tables_for(tets)
        edges = dg.unique_edges(tets).cpu()
        assert torch.equal(tb.edges.cpu().long(), edges)
        _DEV[name] = dict(c=c, pos=c.pos.cuda(), tets=tets, dm=dm, tables=tb, edges=edges, oracle={})
    return _DEV[name]


def _oracle(name, fname, sdf):
    """The oracle's mesh of a field of a case, computed once."""
    d = _dev(name)
    if fname not in d["oracle"]:
        with np.errstate(all="ignore"):
            d["oracle"][fname] = dmtet_oracle.marching_tets(d["c"].pos.numpy(), sdf.numpy(), d["c"].tets)
    return d["oracle"][fname]


def _np(mesh):
    return tuple(t.detach().cpu().numpy() for t in mesh)


def _bar(unit):
    return max(BAR * unit, FLOOR)


def _report(what, got, unit):
    bar = _bar(unit)
    print(f"  {what}: kernel {got:.3e} unit {unit:.3e} bar {bar:.3e} ratio {got / bar:.3f}")
    return got / bar


# ---------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(GOLD, "tetgrid.npz"))
    return {str(k): (tuple(int(x) for x in c), [str(s) for s in h]) for k, c, h in zip(g["fields"], g["counts"], g["sha"])}


@pytest.mark.parametrize("name", tc.CASES)
def test_forward_equals_the_oracle_bit_for_bit(hip_lib, gold, name):
    from meshdiffusion_amd.dmtet import marching_tets_batch
    d = _dev(name)
    c, pos, tets, dm = d["c"], d["pos"], d["tets"], d["dm"]
    fields = tc.forward_fields(c)
    batch, cnt = marching_tets_batch(pos[None].expand(len(fields), -1, -1), torch.stack(list(fields.values())).cuda(), d["tables"])
    assert len(batch) == len(fields) and cnt.shape == (len(fields), 4)
    pinned = 0
    for m, (fname, sdf) in enumerate(fields.items()):
        vo, fo, fto = _oracle(name, fname, sdf)
        nt = tc.NUM_TRI[tc.tet_sign_cases(sdf.numpy(), c.tets)]
        n1, n2 = int((nt == 1).sum()), int((nt == 2).sum())
        v, f, uvs, uv_idx, ftet, vvi = dm(pos, sdf.cuda(), tets)
        assert v.dtype == torch.float32 and f.dtype == torch.int64 and ftet.dtype == torch.int64
        assert tc.same_mesh(_np((v, f, ftet)), (vo, fo, fto)), (name, fname, "DMTet()")
        assert tc.same_mesh(_np(batch[m]), (vo, fo, fto)), (name, fname, "marching_tets_batch")
        assert tuple(int(x) for x in cnt[m]) == (vo.shape[0], fo.shape[0], n1, n2), (name, fname)
        want_uv, want_vvi = tc.uv_idx_of(fto, n1, c.T), tc.valid_vert_idx_of(fto, c.tets)
        assert np.array_equal(uv_idx.cpu().numpy(), want_uv) and np.array_equal(vvi.cpu().numpy(), want_vvi), (name, fname)
        key = f"{name}/{fname}"
        if key in gold:                                            # the unmodified reference's hashes: oracle and kernel
            counts, (h_f, h_v, h_uv, h_vvi) = gold[key]
            assert counts == (vo.shape[0], fo.shape[0])
            assert _sha(fo) == h_f and _sha(vo) == h_v and _sha(want_uv) == h_uv and _sha(want_vvi) == h_vvi, key
            assert _sha(f.cpu().numpy()) == h_f and _sha(v.cpu().numpy()) == h_v, key
            assert _sha(uv_idx.cpu().numpy()) == h_uv and _sha(vvi.cpu().numpy()) == h_vvi, key
            pinned += 1
    print(f"\n{name}: {len(fields)} fields bit-equal to the oracle, {pinned} of them pinned to the reference's hashes; "
          f"last field V {vo.shape[0]} F {fo.shape[0]} (one-triangle tets {n1}, two-triangle tets {n2})")
    if name != "two-pass":                                         # every field with a surface is pinned
        assert pinned == sum(1 for s in fields.values() if (tc.tet_sign_cases(s.numpy(), c.tets) % 15 > 0).any())


@pytest.mark.parametrize("name", ("two-pass", "E1025"))
def test_meshes_of_a_batch_do_not_see_each_other(hip_lib, name):
    from meshdiffusion_amd.dmtet import marching_tets_batch
    d = _dev(name)
    c, tb = d["c"], d["tables"]
    g = torch.Generator().manual_seed(41)
    other = (20.3 - torch.from_numpy(c.lattice[:, 2]) + 1.5 * torch.randn(c.N, generator=g)) if name == "two-pass" else tc.sdf_randn(c, 7)
    sdf = torch.stack([tc.sdf_randn(c), torch.ones(c.N), other]).cuda()
    pos = torch.stack([d["pos"], d["pos"] + 0.05, d["pos"] - 0.05])
    batch, cnt = marching_tets_batch(pos, sdf, tb)
    cnt = np.asarray(cnt).copy()
    assert tuple(cnt[1]) == (0, 0, 0, 0) and cnt[0, 0] > 0 and cnt[2, 0] > 0 and tuple(cnt[0]) != tuple(cnt[2])
    for m in range(3):
        one, c1 = marching_tets_batch(pos[m:m + 1].contiguous(), sdf[m:m + 1].contiguous(), tb)
        assert tuple(np.asarray(c1)[0]) == tuple(cnt[m])
        for a, b in zip(batch[m], one[0]):
            assert a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                      b.view(torch.int32) if b.dtype == torch.float32 else b), m
    assert tc.same_mesh(_np(batch[0]), _oracle(name, "surface" if name == "two-pass" else "randn", tc.sdf_randn(c)))
    print(f"\n{name}: counts {cnt.tolist()}")


def test_stale_workspace_contents_do_not_matter(hip_lib):
    """The per-stream workspace keeps the larger buffer: two-pass, then one-tet, then two-pass again, on one stream."""
    from meshdiffusion_amd.dmtet import _MT_WORKSPACE, marching_tets_batch
    big, small = _dev("two-pass"), _dev("one-tet")
    sdf_big = tc.sdf_randn(big["c"]).cuda()[None]
    sdf_small = tc.sign_patterns()[5].cuda()[None]
    with torch.no_grad():
        first, c1 = marching_tets_batch(big["pos"][None], sdf_big, big["tables"])
        first = [t.clone() for t in first[0]]
        key = (big["pos"].device.index, torch.cuda.current_stream().cuda_stream)
        buf = _MT_WORKSPACE[key]
        mid, c2 = marching_tets_batch(small["pos"][None], sdf_small, small["tables"])
        mid = _np(mid[0])
        assert _MT_WORKSPACE[key] is buf                                       # the small call ran inside the big call's buffer
        third, c3 = marching_tets_batch(big["pos"][None], sdf_big, big["tables"])
    assert tuple(np.asarray(c1)[0]) == tuple(np.asarray(c3)[0]) and tuple(np.asarray(c2)[0]) == (4, 2, 0, 1)
    for a, b in zip(first, third[0]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert tc.same_mesh(mid, _oracle("one-tet", "sign5", tc.sign_patterns()[5]))
    assert tc.same_mesh(_np(third[0]), _oracle("two-pass", "surface", tc.sdf_randn(big["c"])))


def test_too_many_meshes_is_unsupported(hip_lib):
    """gridDim.y ends at 65535: one mesh more is MD_ERR_UNSUPPORTED, answered before any launch (the outputs, 4.7 MB, are already
    allocated by then); the stream is intact afterwards and 65535 meshes, the largest call, are all correct."""
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.dmtet import marching_tets_batch
    d = _dev("one-tet")
    M = 65536
    pos = d["pos"][None].expand(M, -1, -1)
    sdf = tc.sign_patterns()[3].cuda()[None].expand(M, -1)
    with pytest.raises(_lib.MeshDiffusionHipError, match=f"md_marching_tets failed with code {_lib.ERR_UNSUPPORTED}$"):
        marching_tets_batch(pos, sdf, d["tables"])
    torch.cuda.synchronize()
    batch, cnt = marching_tets_batch(pos[:M - 1], sdf[:M - 1], d["tables"])   # 65535 meshes: the largest supported call
    cnt = np.asarray(cnt)
    assert (cnt == np.array([4, 2, 0, 1])).all()
    assert tc.same_mesh(_np(batch[M - 2]), _oracle("one-tet", "sign3", tc.sign_patterns()[3]))
    bits = batch.verts[:, :4].view(torch.int32)
    assert bool((bits == bits[M - 2:M - 1]).all()) and bool((batch.faces == batch.faces[M - 2:M - 1]).all())
    assert bool((batch.face_tet == 0).all())


# ---------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------
def _grads(d, sdf, G=None, seed=0):
    p = d["pos"].detach().clone().requires_grad_(True)
    s = sdf.detach().clone().requires_grad_(True)
    v = d["dm"](p, s, d["tets"])[0]
    assert v.requires_grad
    if G is None:
        G = dg.case_G(v.shape[0], seed)
    (v * G.cuda()).sum().backward()
    return v.detach(), p.grad, s.grad, G


@pytest.mark.parametrize("name", tc.CASES)
def test_backward_against_float64(hip_lib, name):
    """md_marching_tets_bwd through DMTet(), loss sum(verts * G).  Unit: restated_grads in fp32 on the CPU, same inputs."""
    d = _dev(name)
    c, edges = d["c"], d["edges"]
    sdf = tc.sdf_randn(c)
    v, dpos, dsdf, G = _grads(d, sdf.cuda(), seed=100 + tc.CASES.index(name))
    _, dpos2, dsdf2, _ = _grads(d, sdf.cuda(), G=G)
    assert torch.equal(dpos, dpos2) and torch.equal(dsdf, dsdf2)                          # two runs: bit-identical
    p64, s64 = dg.restated_grads(c.pos, sdf, edges, G)
    p32, s32 = dg.restated_grads(c.pos, sdf, edges, G, dtype=torch.float32)
    print(f"\n{name}: V {v.shape[0]}")
    rp = _report("dpos", dg.rel_l2(dpos, p64), dg.rel_l2(p32, p64))
    rs = _report("dsdf", dg.rel_l2(dsdf, s64), dg.rel_l2(s32, s64))
    assert rp <= 1.0 and rs <= 1.0, (name, rp, rs)
    ce = dg.crossing_edges(sdf, edges)
    quiet = torch.ones(c.N, dtype=torch.bool)
    quiet[ce.reshape(-1)] = False                                                         # no crossing edge: exactly zero
    assert bool(quiet[torch.from_numpy(c.unnamed)].all()) and int(quiet.sum()) >= c.unnamed.size
    assert not bool(dpos.cpu()[quiet].any()) and not bool(dsdf.cpu()[quiet].any())
    assert not bool(p64[quiet].any()) and bool((dpos.cpu()[~quiet] != 0).any(1).all())
    if name == "star":
        print(f"  vertex 0 sums {int((ce[:, 0] == 0).sum())} terms")


# ---------------------------------------------------------------------------------------------------------------
# the regulariser
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ("randn", "zeros"))
@pytest.mark.parametrize("name", REG_CASES)
def test_sdf_reg_loss_against_float64(hip_lib, name, field):
    """Value and gradient; `zeros`: +-0.0 among the values, where the mask is torch.sign's and a zero endpoint counts.
    Unit: restated_sdf_reg in fp32 on the CPU, same inputs."""
    from meshdiffusion_amd.dmtet import sdf_reg_loss
    d = _dev(name)
    c, edges, tb = d["c"], d["edges"], d["tables"]
    sdf = tc.sdf_randn(c) if field == "randn" else tc.zeros_field(c)[0]
    s = sdf.cuda().requires_grad_(True)
    loss = sdf_reg_loss(s, tb.all_edges)
    loss.backward()
    s2 = sdf.cuda().requires_grad_(True)
    sdf_reg_loss(s2, tb).backward()
    assert torch.equal(s.grad, s2.grad)
    l64, g64 = dg.restated_sdf_reg(sdf, edges)
    l32, g32 = dg.restated_sdf_reg(sdf, edges, dtype=torch.float32)
    sg = torch.sign(sdf)
    masked = sg[edges[:, 0]] != sg[edges[:, 1]]
    loss = float(loss.detach())
    print(f"\n{name} {field}: loss {loss:.7f} over {int(masked.sum())} of {edges.shape[0]} edges")
    rv = _report("value", abs(loss - float(l64)) / float(l64), abs(float(l32) - float(l64)) / float(l64))
    rg = _report("grad", dg.rel_l2(s.grad, g64), dg.rel_l2(g32, g64))
    assert rv <= 1.0 and rg <= 1.0, (name, field, rv, rg)
    touched = torch.zeros(c.N, dtype=torch.bool)
    touched[edges[masked].reshape(-1)] = True
    assert not bool(s.grad.cpu()[~touched].any())                                          # no masked edge: exactly zero
    if field == "randn":
        assert bool((s.grad.cpu()[touched] != 0).all())
    else:                                   # at a zero sigmoid - target = +-0.5 per edge, which may cancel; its edges all count
        occ = sdf > 0
        assert int(masked.sum()) > int((occ[edges[:, 0]] != occ[edges[:, 1]]).sum()) or name == "one-tet"
        zero_end = (sdf[edges[:, 0]] == 0) != (sdf[edges[:, 1]] == 0)
        assert int(zero_end.sum()) > 0 and bool(masked[zero_end].all())


# ---------------------------------------------------------------------------------------------------------------
# fixed topology
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", (False, True), ids=("sdf", "fixed_sign"))
@pytest.mark.parametrize("name", tc.CASES)
def test_fixed_topology_plan_equals_marching_tets_bit_for_bit(hip_lib, name, frozen):
    from meshdiffusion_amd.dmtet import FixedTopoPlan, fixed_sign
    d = _dev(name)
    c, pos = d["c"], d["pos"]
    sdf = tc.sdf_randn(c).cuda()
    if frozen:
        sdf = fixed_sign(sdf)
        assert set(sdf.unique().tolist()) == {-1.0, 1.0}
    plan = FixedTopoPlan(d["tables"], pos, sdf)
    v, dpos, _, G = _grads(d, sdf, seed=300 + tc.CASES.index(name))
    p = pos.detach().clone().requires_grad_(True)
    pv = plan.verts(p, sdf)
    (pv * G.cuda()).sum().backward()
    assert plan.n_mesh_verts == v.shape[0] and plan.n_grid_verts == c.N
    assert torch.equal(pv.detach().view(torch.int32), v.view(torch.int32)), name          # the contract of csrc/fixedtopo.hip
    assert torch.equal(p.grad.view(torch.int32), dpos.view(torch.int32)), name
    assert torch.equal(plan.initial_verts.view(torch.int32), v.view(torch.int32))
    vo, fo, fto = dmtet_oracle.marching_tets(c.pos.numpy(), sdf.cpu().numpy(), c.tets)
    assert tc.same_mesh(_np((pv, plan.faces, plan.face_tet)), (vo, fo, fto))
    assert np.array_equal(plan.edge.cpu().numpy(), dg.crossing_edges(sdf.cpu(), d["edges"]).numpy())
    assert not bool(p.grad[torch.from_numpy(c.unnamed).cuda()].any())
    print(f"\n{name} {'fixed_sign' if frozen else 'sdf'}: Vm {plan.n_mesh_verts} F {plan.faces.shape[0]} verts and dpos bit-equal")


# ---------------------------------------------------------------------------------------------------------------
# GridMesher at R = 7
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", tc.GRID_MESHER_KINDS)
def test_grid_mesher_at_R7(hip_lib, kind):
    """Vertices to the <= 1e-6 absolute bar of test_dmtet_batch32_vs_oracle, whose inputs go through the same host arithmetic."""
    from meshdiffusion_amd.dmtet import GridMesher
    v, t, grids = tc.grid_mesher_inputs(kind)
    meshes = GridMesher(v, t, 7, mesh_scale=2.1, deform_scale=2.0)(grids.cuda())
    assert len(meshes) == grids.shape[0]
    for m in range(grids.shape[0]):
        pos, sdf = dmtet_oracle.grid_to_tet_inputs(grids[m].numpy(), v, mesh_scale=2.1, deform_scale=2.0, R=7)
        vo, fo, fto = dmtet_oracle.marching_tets(pos, sdf, t)
        vm, fm, ftm = _np(meshes[m])
        err = float(np.abs(vm - vo).max())
        print(f"\n{kind} mesh {m}: V {vo.shape[0]} F {fo.shape[0]} max |verts - oracle| {err:.3e} (bar 1e-6)")
        assert vo.shape[0] > 50 and np.array_equal(fm, fo) and np.array_equal(ftm, fto) and err <= 1e-6
