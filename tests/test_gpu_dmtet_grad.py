"""Differentiable marching tetrahedra on the GPU: md_marching_tets_bwd and md_sdf_reg_loss(+_bwd) against the float64
restatement of the reference's expressions (tests/dmtet_grad_cases.py) and the reference gradients recorded in
tests/golden/dmtet_grad.npz.

Every bar is the reference's OWN recorded rel-L2 distance from the float64 restatement for that case and quantity, x 4
(the fixture's `<case>/ref_err_*`): nothing here is a constant fitted to what the kernel gives.  Inputs that are not one
of the fixture's cases borrow the bar of the case of the same regime: `sphere` for sign-valued SDFs (|den| = 2 on every
crossing edge), `smooth` for real-valued ones.  Each test prints its figures before it asserts.
"""
import os

import numpy as np
import pytest
import torch

import dmtet_grad_cases as dg
from conftest import GOLD

pytestmark = pytest.mark.gpu
BAR = 4.0


@pytest.fixture(scope="module")
def tet():
    t = np.load(os.path.join(GOLD, "64_tets_cropped.npz"))
    return t["vertices"], t["indices"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "dmtet_grad.npz"))


@pytest.fixture(scope="module")
def grid(tet):
    """(pos [N,3], {case: sdf [N]}, tets int64 [T,4], edges int64 [E,2]) on the GPU."""
    from oracle.gen_golden import dmtet_cases
    verts, idx = tet
    pos, cases = dmtet_cases(verts)
    tets_t = torch.as_tensor(idx, dtype=torch.long).cuda()
    return pos.cuda(), {k: v.cuda() for k, v in cases.items()}, tets_t, dg.unique_edges(tets_t)


def _bars(gold, case):
    return BAR * float(gold[f"{case}/ref_err_dpos"]), BAR * float(gold[f"{case}/ref_err_dsdf"])


def _dmtet_grads(dm, pos, sdf, tets_t, G=None, seed=0, pos_grad=True, sdf_grad=True):
    """Through DMTet()(pos, sdf, tets) as a reference user calls it, loss sum(verts * G)."""
    p = pos.detach().clone().requires_grad_(pos_grad)
    s = sdf.detach().clone().requires_grad_(sdf_grad)
    v = dm(p, s, tets_t)[0]
    assert v.requires_grad and v.grad_fn is not None
    if G is None:
        G = dg.case_G(v.shape[0], seed).cuda()
    (v * G).sum().backward()
    return v.detach(), p.grad, s.grad, G


def _batch_inputs(grid, M=8):
    pos, cases, _, _ = grid
    v = pos                                                          # any smooth field of the vertex positions will do
    r = v.norm(dim=1)
    sdf = torch.stack([0.5 + 0.02 * m - r + 0.1 * torch.sin(11 * v[:, m % 3] + m) for m in range(M)])
    g = torch.Generator().manual_seed(77)
    posb = pos[None] + (torch.rand(M, *pos.shape, generator=g) * 2 - 1).cuda() * 0.004
    return posb.contiguous(), sdf.contiguous()


def _batch_grads(posb, sdfb, tables, Gs=None):
    from meshdiffusion_amd.dmtet import marching_tets_batch
    p, s = posb.detach().clone().requires_grad_(True), sdfb.detach().clone().requires_grad_(True)
    meshes, cnt = marching_tets_batch(p, s, tables)
    if Gs is None:
        Gs = [dg.case_G(int(cnt[m, 0]), 500 + m).cuda() for m in range(len(meshes))]
    loss = sum((meshes[m][0] * Gs[m]).sum() for m in range(len(meshes)))
    loss.backward()
    return p.grad, s.grad, Gs


@pytest.mark.parametrize("case", dg.GRAD_CASES)
def test_gradient_parity_with_the_reference(hip_lib, grid, gold, case):
    from meshdiffusion_amd.dmtet import DMTet
    pos, cases, tets_t, edges = grid
    sdf, N = cases[case], pos.shape[0]
    v, dpos, dsdf, G = _dmtet_grads(DMTet(), pos, sdf, tets_t, seed=gold[f"{case}/seed"])
    assert v.shape[0] == int(gold[f"{case}/V"]) and dpos.shape == pos.shape and dsdf.shape == sdf.shape
    assert dpos.dtype == torch.float32 and dsdf.dtype == torch.float32
    bar_p, bar_s = _bars(gold, case)
    dpos64, dsdf64 = dg.restated_grads(pos, sdf, edges, G)
    ep, es = dg.rel_l2(dpos, dpos64), dg.rel_l2(dsdf, dsdf64)
    rows, rp, rs = dg.fixture_rows(gold, case, N)
    fp, fs = dg.rel_l2(dpos[rows], rp), dg.rel_l2(dsdf[rows], rs)
    print(f"\n{case}: vs float64 dpos {ep:.3e} (x{ep * BAR / bar_p:.2f} of the reference's own) dsdf {es:.3e} "
          f"(x{es * BAR / bar_s:.2f}) | vs reference rows dpos {fp:.3e} dsdf {fs:.3e} | bars {bar_p:.3e} {bar_s:.3e}")
    assert ep <= bar_p and es <= bar_s, (case, ep, es)
    assert fp <= bar_p and fs <= bar_s, (case, fp, fs)
    zp, zs = dg.fixture_zero_rows(gold, case, N)
    assert bool((dpos[zp] == 0).all()) and bool((dsdf[zs] == 0).all()), case     # exactly zero where the reference's is
    if case == "noise":
        d = np.abs(dpos.double().sum(0).cpu().numpy() - gold["noise/dpos_colsum"])
        assert (d <= bar_p * dpos.double().abs().sum(0).cpu().numpy()).all()
        assert abs(float(dsdf.double().sum()) - float(gold["noise/dsdf_sum"])) <= bar_s * float(dsdf.double().abs().sum())


def test_backward_is_deterministic_bit_for_bit(hip_lib, grid):
    from meshdiffusion_amd.dmtet import DMTet, TetTables
    pos, cases, tets_t, _ = grid
    dm = DMTet()
    a = _dmtet_grads(dm, pos, cases["noise"], tets_t, seed=3)
    b = _dmtet_grads(dm, pos, cases["noise"], tets_t, G=a[3])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    tb = TetTables(tets_t, tets_t.device)
    posb, sdfb = _batch_inputs(grid, 8)
    p1, s1, Gs = _batch_grads(posb, sdfb, tb)
    p2, s2, _ = _batch_grads(posb, sdfb, tb, Gs)
    assert torch.equal(p1, p2) and torch.equal(s1, s2) and float(p1.abs().sum()) > 0 and float(s1.abs().sum()) > 0


def test_batch_rows_equal_the_single_mesh_calls(hip_lib, grid, gold):
    from meshdiffusion_amd.dmtet import TetTables
    pos, _, tets_t, edges = grid
    tb = TetTables(tets_t, tets_t.device)
    posb, sdfb = _batch_inputs(grid, 8)
    pb, sb, Gs = _batch_grads(posb, sdfb, tb)
    bar_p, bar_s = _bars(gold, "smooth")
    for m in range(8):
        p1, s1, _ = _batch_grads(posb[m:m + 1], sdfb[m:m + 1], tb, Gs[m:m + 1])
        assert torch.equal(pb[m], p1[0]) and torch.equal(sb[m], s1[0]), m
    for m in (0, 7):
        dpos64, dsdf64 = dg.restated_grads(posb[m], sdfb[m], edges, Gs[m])
        ep, es = dg.rel_l2(pb[m], dpos64), dg.rel_l2(sb[m], dsdf64)
        print(f"\nbatch mesh {m}: V={Gs[m].shape[0]} vs float64 dpos {ep:.3e} dsdf {es:.3e} | bars {bar_p:.3e} {bar_s:.3e}")
        assert ep <= bar_p and es <= bar_s, (m, ep, es)


def test_forward_is_untouched_and_the_workspace_is_owned(hip_lib, grid):
    from meshdiffusion_amd.dmtet import DMTet
    pos, cases, tets_t, _ = grid
    dm = DMTet()
    plain = dm(pos, cases["smooth"], tets_t)
    other = dm(pos, cases["sinus"], tets_t)
    assert not plain[0].requires_grad and plain[0].grad_fn is None
    with torch.no_grad():                                            # grad mode off: today's path even for leaf parameters
        ng = dm(pos.clone().requires_grad_(True), cases["smooth"], tets_t)
    assert not ng[0].requires_grad and torch.equal(ng[0], plain[0])
    p, s = pos.clone().requires_grad_(True), cases["smooth"].clone().requires_grad_(True)
    out = dm(p, s, tets_t)
    assert out[0].requires_grad
    for a, b in zip(out, plain):
        assert a.dtype == b.dtype and torch.equal(a.detach(), b)
    for k in (1, 2, 3, 4, 5):
        assert not out[k].requires_grad
    assert out[1].dtype == torch.int64 and out[4].dtype == torch.int64
    # a no-grad call on the same stream between forward and backward: it must see correct meshes, and the backward of the
    # earlier call must still see its own edge -> vertex table
    again = dm(pos, cases["sinus"], tets_t)
    for a, b in zip(again, other):
        assert torch.equal(a, b)
    G = dg.case_G(out[0].shape[0], 9).cuda()
    (out[0] * G).sum().backward()
    _, dp, ds, _ = _dmtet_grads(dm, pos, cases["smooth"], tets_t, G=G)
    assert torch.equal(p.grad, dp) and torch.equal(s.grad, ds)
    final = dm(pos, cases["smooth"], tets_t)
    for a, b in zip(final, plain):
        assert torch.equal(a, b)


def test_edges_of_the_domain(hip_lib, grid, gold):
    from meshdiffusion_amd.dmtet import DMTet
    pos, cases, tets_t, edges = grid
    N = pos.shape[0]
    dm = DMTet()
    for sign in (1.0, -1.0):                                          # no crossing edge at all
        v, dp, ds, _ = _dmtet_grads(dm, pos, torch.full((N,), sign, device="cuda"), tets_t)
        assert v.shape == (0, 3) and dp.shape == pos.shape and not bool(dp.any()) and not bool(ds.any())
    tb = dm.tables_for(tets_t)
    inc_ptr, _ = tb.incidence(N)
    k = int(torch.nonzero((inc_ptr[1:] - inc_ptr[:-1]) == 14)[0, 0])
    one = torch.full((N,), -1.0, device="cuda")
    one[k] = 1.0                                                      # one inside vertex of degree 14
    v, dp, ds, G = _dmtet_grads(dm, pos, one, tets_t, seed=21)
    bar_p, bar_s = _bars(gold, "sphere")
    dp64, ds64 = dg.restated_grads(pos, one, edges, G)
    print(f"\none vertex: V={v.shape[0]} dpos {dg.rel_l2(dp, dp64):.3e} dsdf {dg.rel_l2(ds, ds64):.3e} | bars {bar_p:.3e} {bar_s:.3e}")
    assert v.shape[0] == 14 and int((dp != 0).any(1).sum()) == 15 and int((ds != 0).sum()) == 15
    assert dg.rel_l2(dp, dp64) <= bar_p and dg.rel_l2(ds, ds64) <= bar_s
    # a non-contiguous pos, and one input without a gradient
    sdf = cases["smooth"]
    _, dp, ds, G = _dmtet_grads(dm, pos, sdf, tets_t, seed=22)
    wide = torch.zeros(N, 4, device="cuda")
    wide[:, :3] = pos
    p = wide.requires_grad_(True)
    s = sdf.clone().requires_grad_(True)
    view = p[:, :3]
    assert not view.is_contiguous()
    (dm(view, s, tets_t)[0] * G).sum().backward()
    assert torch.equal(p.grad[:, :3], dp) and not bool(p.grad[:, 3].any()) and torch.equal(s.grad, ds)
    _, dp1, ds1, _ = _dmtet_grads(dm, pos, sdf, tets_t, G=G, pos_grad=False)
    assert dp1 is None and torch.equal(ds1, ds)
    _, dp2, ds2, _ = _dmtet_grads(dm, pos, sdf, tets_t, G=G, sdf_grad=False)
    assert ds2 is None and torch.equal(dp2, dp)


def test_non_finite_sdf_values_stay_local(hip_lib, grid, gold):
    """NaN / inf SDF entries: the call returns, and every vertex whose own and whose neighbours' values are finite gets the
    restatement's gradient."""
    from meshdiffusion_amd.dmtet import DMTet
    pos, cases, tets_t, edges = grid
    N = pos.shape[0]
    sdf = cases["smooth"].clone()
    bad = torch.arange(100, N, 997, device="cuda")
    sdf[bad[0::3]] = float("nan")
    sdf[bad[1::3]] = float("inf")
    sdf[bad[2::3]] = float("-inf")
    v, dp, ds, G = _dmtet_grads(DMTet(), pos, sdf, tets_t, seed=31)
    torch.cuda.synchronize()
    dirty = torch.zeros(N, dtype=torch.bool, device="cuda")
    dirty[bad] = True
    touch = dirty[edges[:, 0]] | dirty[edges[:, 1]]
    dirty[edges[touch].reshape(-1)] = True
    clean = ~dirty
    dp64, ds64 = dg.restated_grads(pos, sdf, edges, G)
    bar_p, bar_s = _bars(gold, "smooth")
    ep, es = dg.rel_l2(dp[clean], dp64[clean]), dg.rel_l2(ds[clean], ds64[clean])
    print(f"\nnon-finite: V={v.shape[0]} clean rows {int(clean.sum())} dpos {ep:.3e} dsdf {es:.3e} | bars {bar_p:.3e} {bar_s:.3e}")
    assert bool(torch.isfinite(dp[clean]).all()) and bool(torch.isfinite(ds[clean]).all())
    assert ep <= bar_p and es <= bar_s


def test_grid_mesher_passes_the_gradient_to_the_deformation_channels(hip_lib, tet, grid, gold):
    from meshdiffusion_amd.dmtet import GridMesher
    verts, idx = tet
    _, _, _, edges = grid
    M, R = 2, 64
    g = torch.Generator().manual_seed(12)
    ax = torch.linspace(-1, 1, R)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    grids = torch.empty(M, 4, R, R, R)
    for m in range(M):
        grids[m, 0] = 0.5 + 0.1 * m - (X ** 2 + Y ** 2 + Z ** 2).sqrt() + 0.05 * torch.sin(9 * X + m)
        grids[m, 1:] = torch.randn(3, R, R, R, generator=g) * 0.7
    mesher = GridMesher(verts, idx, R)
    plain = mesher(grids.cuda())
    gr = grids.cuda().requires_grad_(True)
    meshes = mesher(gr)
    Gs = [dg.case_G(meshes[m][0].shape[0], 600 + m).cuda() for m in range(M)]
    sum((meshes[m][0] * Gs[m]).sum() for m in range(M)).backward()
    for m in range(M):
        assert torch.equal(meshes[m][0].detach(), plain[m][0]) and torch.equal(meshes[m][1], plain[m][1])
    pos, sdf = mesher.inputs(grids.cuda())
    i0, i1, i2 = mesher.idx[:, 0], mesher.idx[:, 1], mesher.idx[:, 2]
    want = torch.zeros(M, 4, R, R, R, dtype=torch.float64, device="cuda")
    scale = 2 / (R * 2) * mesher.deform_scale
    for m in range(M):
        dpos64, _ = dg.restated_grads(pos[m], sdf[m], edges, Gs[m])
        raw = grids[m, 1:].cuda()[:, i0, i1, i2]                                           # [3,N]
        wm = want[m]
        wm[1:, i0, i1, i2] = (dpos64.transpose(0, 1) * scale) * (raw.abs() <= 1.0)
    bar_p, _ = _bars(gold, "sphere")
    e = dg.rel_l2(gr.grad, want)
    print(f"\nGridMesher: dgrids vs float64 {e:.3e} | bar {bar_p:.3e}")
    assert e <= bar_p
    assert not bool(gr.grad[:, 0].any())                                                     # through sign: exactly zero
    outside = (grids[:, 1:].abs() > 1.0).cuda()
    assert int(outside.sum()) > 1000 and not bool(gr.grad[:, 1:][outside].any())
    assert float(gr.grad[:, 1:].abs().sum()) > 0


@pytest.mark.parametrize("case", dg.REG_CASES)
def test_sdf_reg_loss_value_and_gradient(hip_lib, grid, gold, case):
    from meshdiffusion_amd.dmtet import TetTables, sdf_reg_loss
    pos, cases, tets_t, edges = grid
    tb = TetTables(tets_t, tets_t.device)
    sdf = cases[case]

    def run(all_edges):
        s = sdf.clone().requires_grad_(True)
        loss = sdf_reg_loss(s, all_edges)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
        loss.backward()
        return loss.detach(), s.grad

    loss, grad = run(tb.all_edges)
    for other in (tb.all_edges, tb, edges):                         # bit-equal again, and by every way of naming the edges
        l2, g2 = run(other)
        assert torch.equal(loss, l2) and torch.equal(grad, g2)
    loss64, grad64 = dg.restated_sdf_reg(sdf, edges)
    bar_v, bar_g = BAR * float(gold[f"reg/{case}/ref_err_value"]), BAR * float(gold[f"reg/{case}/ref_err_grad"])
    ev = abs(float(loss) - float(loss64)) / float(loss64)
    fv = abs(float(loss) - float(gold[f"reg/{case}/value"])) / float(gold[f"reg/{case}/value"])
    eg = dg.rel_l2(grad, grad64)
    rows = gold[f"reg/{case}/rows"].astype(np.int64)
    fg = dg.rel_l2(grad[rows], gold[f"reg/{case}/grad"])
    print(f"\nsdf_reg_loss {case}: {float(loss):.7f} value vs float64 {ev:.3e} vs reference {fv:.3e} (bar {bar_v:.3e}) | "
          f"grad vs float64 {eg:.3e} vs reference rows {fg:.3e} (bar {bar_g:.3e})")
    assert abs(float(loss64) - float(gold[f"reg/{case}/value64"])) <= 1e-12 * float(loss64)
    assert ev <= bar_v and fv <= bar_v and eg <= bar_g and fg <= bar_g
    assert int((grad != 0).sum()) == int(gold[f"reg/{case}/n_nonzero"])
    assert abs(float(grad.double().sum()) - float(gold[f"reg/{case}/grad_sum"])) <= bar_g * float(grad.double().abs().sum())
    # a scaled loss reads the incoming gradient from the device
    s = sdf.clone().requires_grad_(True)
    (sdf_reg_loss(s, tb.all_edges) * 0.25).backward()
    assert torch.equal(s.grad, grad * 0.25)


def test_sdf_reg_loss_empty_mask_is_the_reference_nan(hip_lib, grid):
    """No edge changes sign: the reference takes the mean of an empty tensor, nan, and its gradient is all zeros."""
    from meshdiffusion_amd.dmtet import TetTables, sdf_reg_loss
    pos, _, tets_t, edges = grid
    tb = TetTables(tets_t, tets_t.device)
    s = torch.full((pos.shape[0],), 0.7, device="cuda").requires_grad_(True)
    loss = sdf_reg_loss(s, tb.all_edges)
    loss.backward()
    loss64, grad64 = dg.restated_sdf_reg(s, edges)
    assert bool(torch.isnan(loss64)) and bool(torch.isnan(loss))
    assert torch.equal(s.grad.double(), grad64) and not bool(s.grad.any())
    with pytest.raises(Exception):
        sdf_reg_loss(torch.zeros(8), tb.all_edges)                  # no CPU path


def test_fit_end_to_end(hip_lib, tet, gold):
    """Fit a sphere of radius 0.6 from a sphere of radius 0.45 with the reference's loop (Adam on sdf and deform, data loss
    + 0.01 * sdf_reg_loss, 41 steps) and carry the result through state_to_dict -> tet_to_grid -> GridMesher.

    Trajectory bar per step: the reference's recorded fp32-vs-fp64 gap at that step x 10, floor 1e-3 (Adam divides by
    sqrt(v): single-ulp gradient differences are amplified early on)."""
    from meshdiffusion_amd import mesh_export
    from meshdiffusion_amd.dmtet import DMTet, DMTetGeometry, GridMesher, sdf_reg_loss, tet_vertices_to_grid_index
    verts, idx = tet
    geo = DMTetGeometry(64, 2.1, None, tets=(verts, idx), deform_scale=2.0)
    assert geo.sdf.shape == (verts.shape[0],) and float(geo.sdf.detach().min()) >= -0.1 and float(geo.sdf.detach().max()) <= 0.9
    assert not bool(geo.deform.any()) and geo.all_edges.shape[1] == 2 and geo.all_edges.dtype == torch.int64
    lo, hi = geo.getAABB()
    assert torch.equal(lo, geo.verts.min(0).values) and torch.equal(hi, geo.verts.max(0).values)
    assert not geo.get_deformed(no_grad=True).requires_grad and geo.get_deformed().requires_grad
    with torch.no_grad():
        geo.sdf.copy_(dg.fit_initial_sdf(geo.verts))
        geo.deform.zero_()
    opt = torch.optim.Adam([geo.sdf, geo.deform], lr=0.01)
    losses, V0 = [], None
    for step in range(41):
        opt.zero_grad()
        mesh = geo.getMesh()
        data = dg.fit_data_loss(mesh.v_pos)
        (data + 0.01 * sdf_reg_loss(geo.sdf, geo.all_edges)).backward()
        opt.step()
        losses.append(float(data))
        if V0 is None:
            V0 = mesh.v_pos.shape[0]
            assert mesh.v_nrm.shape == mesh.v_pos.shape and not mesh.v_nrm.requires_grad
            assert mesh.t_pos_idx.dtype == torch.int64 and mesh.t_tex_idx.shape == mesh.t_pos_idx.shape
            assert mesh.valid_vert_idx.dtype == torch.int64 and mesh.v_tex.shape[1] == 2
    l32, l64 = gold["fit/loss32"], gold["fit/loss64"]
    got = np.array([losses[k] for k in dg.FIT_STEPS])
    rel = np.abs(got - l32) / l32
    tol = np.maximum(10 * np.abs(l32 - l64) / l64, 1e-3)
    print(f"\nfit: V0 {V0} (reference {int(gold['fit/V0'])}) data loss {got} reference {l32} rel {rel} tol {tol}")
    assert V0 == int(gold["fit/V0"])
    assert losses[40] <= 0.01 * losses[0]
    assert (rel[1:] <= tol[1:]).all() and rel[0] <= tol[0]
    # fit -> dict -> training grid -> mesh
    d = geo.state_to_dict()
    assert set(d) == {"sdf", "deform"} and not d["sdf"].is_cuda and not d["sdf"].requires_grad
    g = mesh_export.tet_to_grid(tet_vertices_to_grid_index(torch.as_tensor(verts)), d["sdf"], d["deform"], 64)
    faces = GridMesher(verts, idx, 64)(g[None].cuda())[0][1]
    with torch.no_grad():
        pos = geo.verts + 2 / (64 * 2) * geo.deform.clip(-1.0, 1.0) * 2.0
        want = DMTet()(pos, torch.sign(geo.sdf), geo.indices)[1]
    assert faces.shape[0] > 0 and torch.equal(faces, want)
