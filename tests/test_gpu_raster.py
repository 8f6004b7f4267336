"""The depth rasteriser on the GPU (csrc/raster.hip, meshdiffusion_amd/render.py) against the torch restatements of the
rasterisation contract in tests/raster_cases.py.

Bars, none fitted to what the kernels give:
  face ids      bit-equal to the brute-force restatement (fp32 snap and int64 coverage on the CPU, float64 keys) on every pixel
                whose float64 keys are at least 1e-6 apart; the pixels left out are capped at 0.5 % of the covered ones.
  u, v, zf, depth, d verts   rel-L2 against float64 <= 4 x the fp32 torch restatement's OWN rel-L2 distance from float64 on the
                same case, recorded in tests/golden/raster.npz by tools/gen_golden_raster.py (the margin of
                tests/test_gpu_dmtet_grad.py).  Uncovered pixels hold exactly 0 / 20.0 / -1.0.
  fitting run   4 x |fp32 - float64| of the restated loop at each stored iteration, floored at 1e-6 relative.
Each test prints its figures before it asserts.
"""
import functools
import os

import numpy as np
import pytest
import torch

import raster_cases as rc
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu
BAR = 4.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "raster.npz"))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Per mesh case, computed once and left unchanged: the inputs on the GPU, the restated rasterisation of the SAME pos_clip
    tensor (snap and coverage on the CPU), the exclusions and the float64 values."""
    from meshdiffusion_amd import render
    name, H, W = case
    verts, faces = rc.mesh(name)
    mvp, campos = rc.cameras(rc.ANGLES, H, W)
    verts, faces, mvp, campos = verts.cuda(), faces.cuda(), mvp.cuda(), campos.cuda()
    pc = render.xfm_points(verts[None], mvp).contiguous()
    r = rc.rasterize_restated(pc.cpu(), faces.cpu(), H, W)
    order, numeric, covered = rc.check_caps(r, rc.case_id(case))
    ids = r["ids"].cuda()
    u64, v64 = rc.bary_restated(pc, faces, ids)
    d64 = rc.depth_restated(verts, faces, mvp, campos, ids)
    return dict(verts=verts, faces=faces, mvp=mvp, campos=campos, pc=pc, ids=ids, zf=r["zf"].cuda(), u=u64, v=v64, depth=d64,
                order=order.cuda(), use=(covered & ~order & ~numeric).cuda(), H=H, W=W)


def _ids_of(rast):
    assert all(t.dtype == torch.float32 for t in rast)
    return torch.stack([t[..., 3] for t in rast], 1).to(torch.int64)


@pytest.mark.parametrize("name", rc.SMALL_CASES)
def test_face_ids_small_cases(hip_lib, name):
    from meshdiffusion_amd import render
    pc, faces, H, W = rc.small_case(name)
    r = rc.rasterize_restated(pc, faces, H, W)
    rast = render.rasterize(pc.cuda(), faces.cuda(), (H, W))
    assert len(rast) == 2 and all(t.shape == (1, H, W, 4) and not t.requires_grad for t in rast)
    ids = _ids_of(rast).cpu()
    print(f"\n{name}: covered {int((r['ids'][:, 0] > 0).sum())} / {int((r['ids'][:, 1] > 0).sum())} centres on edges {r['on_edge']}")
    assert torch.equal(ids, r["ids"]), name
    if name == "quad":
        assert r["on_edge"] > 0 and int((ids[0, 0] > 0).sum()) == 25
    if name == "huge":
        assert bool((ids[0, 0] == 1).all()) and not bool(ids[0, 1].any())
    if name == "skipped":
        assert set(ids.unique().tolist()) == {0, 3}
    if name == "empty":
        assert not bool(ids.any()) and all(not bool(t.any()) for t in rast)
    if name == "coincident":
        cov = ids[0, 0] > 0
        assert int(cov.sum()) > 10 and bool((ids[0, 0][cov] == 1).all()) and bool((ids[0, 1][cov] == 2).all())
        assert torch.equal(rast[0][..., :3], rast[1][..., :3])
    assert len(render.rasterize(pc.cuda(), faces.cuda(), (H, W), num_layers=1)) == 1


@pytest.mark.parametrize("case", rc.MESH_CASES, ids=rc.case_id)
def test_face_ids_and_values_on_meshes(hip_lib, gold, case):
    from meshdiffusion_amd import render
    ref = _reference(case)
    cid, H, W = rc.case_id(case), ref["H"], ref["W"]
    rast = render.rasterize(ref["pc"], ref["faces"], (H, W))
    ids = _ids_of(rast)
    keep = ~ref["order"]
    wrong = (ids != ref["ids"]) & keep
    print(f"\n{cid}: id differences outside the left-out set {int(wrong.sum())} (left out {int(ref['order'][:, 1].sum())})")
    assert not bool(wrong.any()), cid
    # values on the pixels not left out
    use = ref["use"]
    got = torch.stack([t[..., :3] for t in rast], 1)                           # [B,2,H,W,3]
    out = render.render_depth(ref["verts"], ref["faces"], ref["mvp"], ref["campos"], (H, W))
    depth = torch.stack([out["depth"][..., 0], out["depth_second"][..., 0]], 1)
    e_uv = rc.rel_l2(torch.stack([got[..., 0], got[..., 1]])[:, use], torch.stack([ref["u"], ref["v"]])[:, use])
    e_zf, e_d = rc.rel_l2(got[..., 2][use], ref["zf"][use]), rc.rel_l2(depth[use], ref["depth"][use])
    units = {k: float(gold[f"case/{cid}/ref_err_{k}"]) for k in ("uv", "zf", "depth")}
    print(f"{cid}: rel-L2 vs float64 / fp32 restatement's own: uv {e_uv:.3e} / {units['uv']:.3e}  zf {e_zf:.3e} / {units['zf']:.3e}  "
          f"depth {e_d:.3e} / {units['depth']:.3e}")
    assert e_uv <= BAR * units["uv"] and e_zf <= BAR * units["zf"] and e_d <= BAR * units["depth"], cid
    # uncovered pixels hold exactly 0 / 20.0 / -1.0, the masks are the coverage
    unc = ids == 0
    assert not bool(torch.stack(rast, 1)[unc].any())
    assert bool((depth[:, 0][unc[:, 0]] == 20.0).all()) and bool((depth[:, 1][unc[:, 1]] == -1.0).all())
    assert torch.equal(out["mask"][..., 0], (~unc[:, 0]).float()) and torch.equal(out["mask_second"][..., 0], (~unc[:, 1]).float())
    assert bool(unc.any()) and bool((~unc[:, 1]).any())


@pytest.mark.parametrize("case", rc.GRAD_CASES, ids=rc.case_id)
def test_vertex_gradient_against_float64_autograd(hip_lib, gold, case):
    from meshdiffusion_amd import render
    ref = _reference(case)
    cid, H, W = rc.case_id(case), ref["H"], ref["W"]
    G = (rc.case_G(tuple(ref["ids"].shape), int(gold["case/g_seed"])).cuda() * ref["use"]).float()
    g64 = rc.grad_restated(ref["verts"], ref["faces"], ref["mvp"], ref["campos"], ref["ids"], G)
    grads = []
    for _ in range(2):
        v = ref["verts"].clone().requires_grad_(True)
        out = render.render_depth(v, ref["faces"], ref["mvp"], ref["campos"], (H, W))
        assert out["depth"].grad_fn is not None and out["depth_second"].grad_fn is not None
        ((out["depth"][..., 0] * G[:, 0]).sum() + (out["depth_second"][..., 0] * G[:, 1]).sum()).backward()
        grads.append(v.grad)
    err, unit = rc.rel_l2(grads[0], g64), float(gold[f"case/{cid}/ref_err_dverts"])
    ids = _ids_of([out["rast"], out["rast_second"]])
    touched = torch.zeros(ref["verts"].shape[0], dtype=torch.bool, device="cuda")
    touched[ref["faces"][ids[ids > 0] - 1].reshape(-1)] = True
    print(f"\n{cid}: d verts rel-L2 vs float64 {err:.3e}, fp32 restatement's own {unit:.3e}; vertices of visible faces "
          f"{int(touched.sum())} of {touched.numel()}")
    assert grads[0].dtype == torch.float32 and grads[0].shape == ref["verts"].shape and bool(torch.isfinite(grads[0]).all())
    assert torch.equal(grads[0], grads[1])                                     # a gather: bit-identical runs
    assert not bool(grads[0][~touched].any()) and bool((~touched).any())
    assert err <= BAR * unit, cid


def test_render_depth_wiring(hip_lib):
    from meshdiffusion_amd import render
    ref = _reference(rc.MESH_CASES[2])
    H, W = ref["H"], ref["W"]
    out = render.render_depth(ref["verts"][None], ref["faces"], ref["mvp"], ref["campos"], (H, W))
    assert set(out) == {"depth", "depth_second", "mask", "mask_second", "rast", "rast_second", "rast_triangle_id"}
    rast = render.rasterize(render.xfm_points(ref["verts"][None], ref["mvp"]), ref["faces"], (H, W))
    assert torch.equal(out["rast"], rast[0]) and torch.equal(out["rast_second"], rast[1])
    ids = rast[0][..., 3].to(torch.int64)
    want = torch.unique(ids[ids > 0] - 1)
    assert out["rast_triangle_id"].dtype == torch.int64 and torch.equal(out["rast_triangle_id"], want)
    for k in ("depth", "depth_second", "mask", "mask_second"):
        assert out[k].shape == (2, H, W, 1) and out[k].grad_fn is None and not out[k].requires_grad, k
    # nothing visible: background everywhere, no ids
    away = render.render_depth(ref["verts"] + 100.0, ref["faces"], ref["mvp"], ref["campos"], (H, W))
    assert away["rast_triangle_id"] is None and bool((away["depth"] == 20.0).all()) and bool((away["depth_second"] == -1.0).all())
    tgt = render.make_targets(ref["verts"], ref["faces"], ref["mvp"], ref["campos"], (H, W))
    assert set(tgt) == {"depth", "depth_second", "mask_cont", "mvp", "campos", "resolution"} and tgt["resolution"] == [H, W]
    assert torch.equal(tgt["depth"], out["depth"]) and torch.equal(tgt["mask_cont"], out["mask"])
    assert float(render.depth_loss(out, tgt, 0)) == 0.0


def test_fit_to_views_end_to_end(hip_lib, gold):
    """fit_to_views on the shipped 64 tet grid from a sphere of radius 0.9 to the torus: 4 views at 64 x 64, 41 iterations, Adam,
    depth loss + sdf regulariser, no chamfer, no carve.  Bar: within 4 x |fp32 - float64| (floored at 1e-6 relative) of the
    float64 value of the restated loop at iterations 0, 10, 20, 40; the final loss below half the first.  Then one carve."""
    from meshdiffusion_amd import render
    from meshdiffusion_amd.dmtet import DMTetGeometry
    geo = DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(rc.fit_initial_sdf(geo.verts))
        geo.deform.zero_()
    mvp, campos = rc.fit_cameras()
    tv, tf = rc.mesh("torus")
    targets = render.make_targets(tv.cuda(), tf.cuda(), mvp.cuda(), campos.cuda(), rc.FIT_RES)
    seen = []
    hist = render.fit_to_views(geo, targets, rc.FIT_ITERS, lr=rc.FIT_LR, sdf_regularizer=rc.FIT_SDF_REGULARIZER, carve=False,
                               callback=lambda it, loss, mesh: seen.append(it))
    assert hist.shape == (rc.FIT_ITERS,) and hist.dtype == torch.float32 and seen == list(range(rc.FIT_ITERS))
    got = hist.double().cpu().numpy()[list(rc.FIT_STEPS)]
    l32, l64 = gold["fit/loss32"], gold["fit/loss64"]
    unit = np.maximum(np.abs(l32 - l64), 1e-6 * np.abs(l64))
    ratio = np.abs(got - l64) / unit
    print(f"\nfit: depth loss {got} float64 restated loop {l64} fp32 restated loop {l32} |gpu - f64| / unit {ratio}")
    # the carve, on the fitted geometry: grid vertices far outside every silhouette are carved, those on the torus's centre
    # circle are not
    sdf_before = geo.sdf.detach().clone()
    n = render.carve_outside_silhouette(geo, targets)
    p = geo.verts
    ring = torch.sqrt((torch.sqrt(p[:, 0] ** 2 + p[:, 2] ** 2) - 0.6) ** 2 + p[:, 1] ** 2)
    carved = (geo.sdf.detach() == 1e-2) & (geo.deform.detach() == 0).all(1)
    print(f"carve: {n} of {p.shape[0]} grid vertices")
    assert 0 < n < p.shape[0] and int(carved.sum()) >= n
    assert bool(carved[p.norm(dim=1) > 1.5].all()) and bool((p.norm(dim=1) > 1.5).any())
    assert torch.equal(geo.sdf.detach()[ring < 0.1], sdf_before[ring < 0.1]) and bool((ring < 0.1).any())
    d = geo.state_to_dict()
    assert set(d) == {"sdf", "deform"}
    assert got[3] < 0.5 * got[0]
    assert (ratio <= BAR).all()


def test_fit_views_tool_writes_a_dict_that_dicts_to_grids_reads(hip_lib, tmp_path):
    """tools/fit_views.py in this process: .obj -> targets -> three iterations -> dmt_dict -> grid."""
    import importlib.util
    from meshdiffusion_amd import mesh_export
    spec = importlib.util.spec_from_file_location("fit_views", os.path.join(ROOT, "tools", "fit_views.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tv, tf = rc.mesh("torus")
    obj = str(tmp_path / "torus.obj")
    mesh_export.save_obj(obj, tv, tf)
    out = str(tmp_path / "fitted" / "dmt_dict_00000.pt")
    tool.main(["--obj", obj, "--tet_path", os.path.join(GOLD, "64_tets_cropped.npz"), "--views", "4", "--res", "32",
               "--views_per_iter", "2", "--iters", "3", "--sphere_init", "0.9", "--points", "2000", "--out", out])
    d = torch.load(out, map_location="cpu", weights_only=False)
    n = rc.tet_grid()[0].shape[0]
    assert set(d) == {"sdf", "deform"} and d["sdf"].shape == (n,) and d["deform"].shape == (n, 3)
    written = mesh_export.dicts_to_grids(rc.tet_grid()[0], str(tmp_path / "fitted"), str(tmp_path / "grids"), 64, [0])
    assert len(written) == 1
    grid = torch.load(written[0], map_location="cpu", weights_only=False)
    assert tuple(grid.shape) == (4, 64, 64, 64) and bool(torch.isfinite(grid).all()) and bool(grid[0].any())
