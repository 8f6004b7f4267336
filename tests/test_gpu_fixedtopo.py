"""The fixed-topology second pass on the GPU (csrc/fixedtopo.hip, dmtet.FixedTopoPlan, dmtet.DMTetGeometryFixedTopo,
render.laplace_regularizer_const, render.fit_fixed_topology, tools/fit_views.py --pass2_iters) against the existing marching
tetrahedra and the restatements of tests/fixedtopo_cases.py.

Bars, none fitted to what the kernels give:
  plan vertices, d deform, the loop without the Laplacian   torch.equal with the existing path (md_marching_tets and its backward).
  Laplacian value and d x     rel-L2 against the float64 restatement <= 4 x the fp32 torch restatement's OWN rel-L2 distance from
                    float64 for that mesh, recorded in tests/golden/fixedtopo.npz by tools/gen_golden_fixedtopo.py (the margin of
                    tests/test_gpu_interp.py); the unit of the scalar value is at least 2^-24, half an ulp of its float32.
  Laplacian term inside the loop   the same bar with the unit computed on the spot, for the vertices the callback hands over; a
                    float64 value of exactly 0 (iteration 0: nothing has moved) demands exactly 0.
Each test prints its figures before it asserts.
"""
import functools
import os

import numpy as np
import pytest
import torch

import fixedtopo_cases as fc
import raster_cases as rc
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "fixedtopo.npz"))


@functools.lru_cache(maxsize=None)
def _grid():
    """The shipped 64 grid on the device, computed once and left unchanged: (pos [N,3], tets int64 [T,4], TetTables)."""
    from meshdiffusion_amd.dmtet import TetTables
    verts, idx = rc.tet_grid()
    pos = (torch.as_tensor(verts, dtype=torch.float32) * rc.MESH_SCALE).cuda()
    tets = torch.as_tensor(idx, dtype=torch.long).cuda()
    return pos, tets, TetTables(tets, tets.device)


def _deformed(pos, deform):
    return pos + 2 / (64 * 2) * deform * 2.0


@pytest.mark.parametrize("case", fc.SDF_CASES)
def test_plan_against_marching_tetrahedra(hip_lib, case):
    from meshdiffusion_amd import dmtet
    pos0, tets, tb = _grid()
    sdf, deform = (x.cuda() for x in fc.sdf_case(case))
    N = pos0.shape[0]
    plan = dmtet.FixedTopoPlan(tb, _deformed(pos0, deform), sdf)
    want = dmtet.DMTet()(_deformed(pos0, deform), sdf, tets)
    Vm, F = plan.n_mesh_verts, plan.faces.shape[0]
    G = torch.randn(Vm, 3, generator=torch.Generator().manual_seed(11)).cuda()
    gen = torch.Generator().manual_seed(12)
    print(f"\nplan {case}: N {N} Vm {Vm} F {F} largest grid-vertex row {int((plan.inc_ptr[1:] - plan.inc_ptr[:-1]).max())}")
    assert torch.equal(plan.faces, want[1]) and torch.equal(plan.uvs, want[2]) and torch.equal(plan.uv_idx, want[3])
    assert torch.equal(plan.face_tet, want[4]) and torch.equal(plan.valid_vert_idx, want[5])
    assert plan.edge.shape == (Vm, 2) and plan.edge.dtype == torch.int32 and plan.inc.shape == (2 * Vm,)
    assert plan.neighbours.shape == (F, 3) and plan.corner_csr[0].shape == (Vm + 1,) and plan.corner_csr[1].shape == (3 * F,)
    for unit in (True, False):                                          # |sdf| = 1, then |sdf| random in [0.1, 1]
        s = sdf if unit else sdf * (0.1 + 0.9 * torch.rand(N, generator=gen)).cuda()
        runs = []
        for _ in range(2):
            d_new = deform.clone().requires_grad_(True)
            v_new = plan.verts(_deformed(pos0, d_new), s)
            assert v_new.grad_fn is not None and v_new.shape == (Vm, 3) and v_new.dtype == torch.float32
            torch.autograd.backward(v_new, G)
            runs.append((v_new.detach(), d_new.grad))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])     # two runs, bit for bit
        d_old = deform.clone().requires_grad_(True)
        s_old = s.clone().requires_grad_(True)
        v_old = dmtet.DMTet()(_deformed(pos0, d_old), s_old, tets)[0]
        torch.autograd.backward(v_old, G)
        v_new, g_new = runs[0]
        n_v, n_g = int((v_new != v_old.detach()).sum()), int((g_new != d_old.grad).sum())
        print(f"  |sdf| {'= 1' if unit else 'in [0.1, 1]'}: verts differing from marching_tets {n_v} of {v_new.numel()}, d deform "
              f"differing {n_g} of {g_new.numel()}, nonzero gradient rows {int(g_new.any(1).sum())}")
        assert torch.equal(v_new, v_old.detach()) and torch.equal(g_new, d_old.grad) and bool(g_new.any())
        if unit:
            p = _deformed(pos0, deform)
            a, b = plan.edge[:, 0].long(), plan.edge[:, 1].long()
            assert torch.equal(v_new, 0.5 * p[a] + 0.5 * p[b])                                  # the exact midpoint
    s = sdf.clone().requires_grad_(True)                                                        # the frozen SDF gets no gradient
    plan.verts(_deformed(pos0, deform.clone().requires_grad_(True)), s).sum().backward()
    assert s.grad is None
    with pytest.raises(ValueError):
        plan.verts(pos0[:-1], sdf[:-1])


@pytest.mark.parametrize("kind", fc.BASES)
@pytest.mark.parametrize("name", fc.LAPLACE_MESHES)
def test_laplacian_against_float64(hip_lib, gold, name, kind):
    from meshdiffusion_amd import dmtet, render
    x, base, faces = fc.laplace_case(name)
    b = base if kind == "base" else None
    v64, g64 = fc.laplace_grads_restated(x, faces, b, torch.float64)
    f_gpu = faces.cuda()
    csr = dmtet.face_corner_csr(f_gpu, x.shape[0])
    runs = []
    for k in range(3):                                                  # the last run with the prebuilt CSR
        xx = x.cuda().requires_grad_(True)
        val = render.laplace_regularizer_const(xx, f_gpu, base=None if b is None else b.cuda(), corner_csr=csr if k == 2 else None)
        assert val.shape == () and val.dtype == torch.float32 and val.grad_fn is not None
        (val * fc.GRAD_OUT).backward()
        runs.append((val.detach(), xx.grad))
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])                  # no atomics: bit-identical runs
    val, dx = runs[0][0].cpu(), runs[0][1].cpu()
    e_v, e_g = rc.rel_l2(val, v64), rc.rel_l2(dx, g64)
    u_v, u_g = float(gold[f"laplace/{name}/{kind}/ref_err_value"]), float(gold[f"laplace/{name}/{kind}/ref_err_dx"])
    print(f"\nlaplace {name} {kind}: V {x.shape[0]} F {faces.shape[0]} value {float(val):.9e} float64 {float(v64):.9e}  rel-L2 vs "
          f"float64 / unit: value {e_v:.2e}/{u_v:.2e}={fc.ratio(e_v, u_v):.2f} d x {e_g:.2e}/{u_g:.2e}={fc.ratio(e_g, u_g):.2f}")
    if name == "degen":                                                 # the unreferenced vertex and the zero-area face: exactly 0
        assert not bool(dx[4:].any()) and bool(dx[:4].any())
    if name == "fan40":
        assert int((faces == 0).sum()) == 40 and bool(dx[0].any())
    assert fc.within(e_v, u_v) and fc.within(e_g, u_g)


def _sphere_geometry():
    """A sphere-initialised DMTetGeometry on the shipped grid (radius rc.FIT_START_RADIUS) with a small seeded deform."""
    from meshdiffusion_amd.dmtet import DMTetGeometry
    geo = DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(rc.fit_initial_sdf(geo.verts))
        geo.deform.copy_((torch.rand(geo.verts.shape, generator=torch.Generator().manual_seed(21)) * 0.2 - 0.1).cuda())
    return geo


@functools.lru_cache(maxsize=None)
def _targets():
    from meshdiffusion_amd import render
    mvp, campos = rc.cameras(rc.FIT_ANGLES, fc.LOOP_RES, fc.LOOP_RES)
    tv, tf = rc.mesh("torus")
    return render.make_targets(tv.cuda(), tf.cuda(), mvp.cuda(), campos.cuda(), fc.LOOP_RES, antialias=True)


def test_geometry_and_loop_without_the_laplacian_are_bit_equal_to_the_existing_path(hip_lib):
    from meshdiffusion_amd import dmtet, render
    first = _sphere_geometry()
    geo = dmtet.DMTetGeometryFixedTopo(first, 64, rc.MESH_SCALE, deform_scale=2.0)
    geo.set_init_v_pos()
    sign = geo.sdf_sign.detach().clone()
    assert not geo.sdf_sign.requires_grad and not geo.sdf_abs.requires_grad and geo.deform.requires_grad
    assert bool((sign.abs() == 1).all()) and bool((geo.sdf_abs == 1).all()) and torch.equal(geo.deform.detach(), first.deform.detach())
    assert [n for n, p in geo.named_parameters() if p.requires_grad] == ["deform"]
    mesh, old = geo.getMesh(), first.getMesh()
    assert set(vars(mesh)) == set(vars(old))
    assert torch.equal(mesh.t_pos_idx, old.t_pos_idx) and torch.equal(mesh.v_tex, old.v_tex) and torch.equal(mesh.t_tex_idx, old.t_tex_idx)
    assert torch.equal(mesh.valid_vert_idx, old.valid_vert_idx) and torch.equal(geo.getValidVertsIdx(), first.getValidVertsIdx())
    assert torch.equal(geo.getValidTetIdx(), first.getValidTetIdx()) and torch.equal(geo.getTetCenters(), first.getTetCenters())
    assert torch.equal(geo.initial_guess_v_pos, mesh.v_pos.detach()) and geo.getMesh(normals_grad=True).v_nrm.grad_fn is not None
    targets = _targets()
    faces0 = geo.plan.faces.clone()
    seen = []

    def callback(it, loss, m):
        seen.append(bool(torch.equal(m.t_pos_idx, faces0)))

    terms = render.fit_fixed_topology(geo, targets, fc.LOOP_ITERS, lr=fc.LOOP_LR, laplace_scale=0.0, warmup_iter=4, callback=callback)
    # the same loop through the existing path: DMTet() on sign * 1 every iteration, the same renderer calls, the same optimizer
    deform = torch.nn.Parameter(first.deform.detach().clone())
    mt = dmtet.DMTet()
    opt = torch.optim.Adam([deform], lr=fc.LOOP_LR)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda it: render.lr_schedule_fixedtopo(it, 4))
    local = []
    for it in range(fc.LOOP_ITERS):
        opt.zero_grad(set_to_none=True)
        verts, faces = mt(first.verts + 2 / (64 * 2) * deform * 2.0, sign * 1.0, first.indices)[:2]
        assert torch.equal(faces, faces0)
        buf = render.render_depth(verts, faces, targets["mvp"], targets["campos"], targets["resolution"])
        loss = render.depth_loss_fixedtopo(buf, targets)
        loss.backward()
        opt.step()
        sched.step()
        deform.data[:] = deform.data.clamp(-0.99, 0.99)
        local.append(loss.detach())
    moved = float((geo.deform.detach() - first.deform.detach()).abs().max())
    n_diff = int((geo.deform.detach() != deform.detach()).sum())
    print(f"\nloop: {fc.LOOP_ITERS} iterations, depth term {float(terms[0]):.6f} -> {float(terms[-1]):.6f}, largest |deform - start| "
          f"{moved:.3e}, elements differing from the existing path {n_diff} of {deform.numel()}")
    assert terms.shape == (fc.LOOP_ITERS,) and len(seen) == fc.LOOP_ITERS and all(seen)
    assert moved > 0 and torch.equal(terms, torch.stack(local)) and torch.equal(geo.deform.detach(), deform.detach())
    # assigning a new sign rebuilds the plan
    geo.sdf_sign = -sign
    assert torch.equal(geo.sdf_sign, -sign) and torch.equal(geo.plan.faces.sort(1).values, faces0.sort(1).values)
    assert not torch.equal(geo.plan.faces, faces0)


def test_loop_with_the_laplacian(hip_lib):
    from meshdiffusion_amd import dmtet, render
    geo = dmtet.DMTetGeometryFixedTopo(_sphere_geometry(), 64, rc.MESH_SCALE, deform_scale=2.0)
    geo.set_init_v_pos()
    base = geo.initial_guess_v_pos.cpu()
    kept = {}

    def callback(it, loss, m):
        if it in fc.LOOP_STEPS:
            kept[it] = m.v_pos.detach().cpu()

    terms = render.fit_fixed_topology(geo, _targets(), fc.LOOP_ITERS, lr=fc.LOOP_LR, laplace_scale=10000.0, warmup_iter=4,
                                      callback=callback, return_terms=True)
    assert set(terms) == {"depth", "laplace", "alpha"} and all(t.shape == (fc.LOOP_ITERS,) and t.is_cuda for t in terms.values())
    faces = geo.plan.faces.cpu()
    ok = True
    for it in fc.LOOP_STEPS:
        got = float(terms["laplace"][it])
        v64 = float(fc.laplace_restated(kept[it], faces, base, torch.float64)[0])
        v32 = float(fc.laplace_restated(kept[it], faces, base, torch.float32)[0])
        unit = max(abs(v32 - v64) / abs(v64), fc.HALF_ULP) if v64 != 0 else 0.0
        err = abs(got - v64) / abs(v64) if v64 != 0 else abs(got)
        print(f"\nloop iteration {it}: laplace term {got:.9e} float64 restated {v64:.9e} fp32 restated {v32:.9e} |gpu - f64| / unit "
              f"{fc.ratio(err, unit):.2f}")
        ok = ok and fc.within(err, unit)
    assert float(terms["laplace"][0]) == 0.0 and float(terms["laplace"][fc.LOOP_STEPS[-1]]) > 0
    assert ok


def test_fit_views_tool_with_the_second_pass(hip_lib, tmp_path):
    """tools/fit_views.py --pass2_iters 3 in this process at --res 32."""
    import importlib.util
    from meshdiffusion_amd import mesh_export
    spec = importlib.util.spec_from_file_location("fit_views", os.path.join(ROOT, "tools", "fit_views.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tv, tf = rc.mesh("torus")
    obj = str(tmp_path / "torus.obj")
    mesh_export.save_obj(obj, tv, tf)
    common = ["--obj", obj, "--tet_path", os.path.join(GOLD, "64_tets_cropped.npz"), "--views", "4", "--res", "32",
              "--views_per_iter", "2", "--iters", "3", "--sphere_init", "0.9"]
    out = str(tmp_path / "fitted" / "dmt_dict_00000.pt")
    tool.main(common + ["--pass2_iters", "3", "--out", out])
    plain = str(tmp_path / "plain" / "dmt_dict_00000.pt")
    tool.main(common + ["--out", plain])
    assert not os.path.exists(str(tmp_path / "plain" / "tets_pre"))
    d = torch.load(out, map_location="cpu", weights_only=False)
    pre = torch.load(str(tmp_path / "fitted" / "tets_pre" / "dmt_dict_00000.pt"), map_location="cpu", weights_only=False)
    one = torch.load(plain, map_location="cpu", weights_only=False)
    n = rc.tet_grid()[0].shape[0]
    assert set(d) == {"sdf", "deform", "deform_unmasked"} and d["sdf"].shape == (n,) and d["deform"].shape == (n, 3)
    assert bool((d["sdf"].abs() == 1).all())
    assert set(pre) == set(one) == {"sdf", "deform"} and torch.equal(pre["sdf"], one["sdf"]) and torch.equal(pre["deform"], one["deform"])
    assert torch.equal(d["sdf"], torch.where(torch.sign(pre["sdf"] + 1e-8) == 0, torch.ones(n), torch.sign(pre["sdf"] + 1e-8)))
    # the mask is getValidVertsIdx() of the written sign: the vertices of the tets the surface passes through
    from meshdiffusion_amd.dmtet import DMTet
    tets = torch.as_tensor(rc.tet_grid()[1], dtype=torch.long).cuda()
    pos = torch.as_tensor(rc.tet_grid()[0], dtype=torch.float32).cuda()
    valid = DMTet()(pos, d["sdf"].cuda(), tets)[5].cpu()
    inside = torch.zeros(n, dtype=torch.bool)
    inside[valid] = True
    print(f"\ntool: {int(inside.sum())} of {n} grid vertices carry a deformation; largest |deform| {float(d['deform'].abs().max()):.3e}")
    assert 0 < int(inside.sum()) < n and not bool(d["deform"][~inside].any()) and torch.equal(d["deform"][inside], d["deform_unmasked"][inside])
    written = mesh_export.dicts_to_grids(rc.tet_grid()[0], str(tmp_path / "fitted"), str(tmp_path / "grids"), 64, [0])
    assert len(written) == 1
    grid = torch.load(written[0], map_location="cpu", weights_only=False)
    assert tuple(torch.as_tensor(grid).shape) == (4, 64, 64, 64)
