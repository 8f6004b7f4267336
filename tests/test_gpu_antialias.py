"""The silhouette antialiasing on the GPU (csrc/antialias.hip, meshdiffusion_amd/render.py) against the restatements of the
antialiasing contract in tests/antialias_cases.py, fed the kernels' own `rast`.

Bars, none fitted to what the kernels give:
  edge neighbours   torch.equal to the numpy restatement.
  pair decisions    active or not, the edge's vertex ids, which pixel is P and which receives: torch.equal to the restatement (int64
                    arithmetic and fp32 on the CPU), no exclusions.
  value, d color, d pos_clip, d verts   rel-L2 against the float64 restatement <= 4 x the fp32 torch restatement's OWN rel-L2
                    distance from float64 for that case, layer, colour and quantity, recorded in tests/golden/antialias.npz by
                    tools/gen_golden_antialias.py (the margin of tests/test_gpu_raster.py).
  fitting run       4 x max(|fp32 loop - float64 loop|, 1e-6 |float64|) of the restated loop at each stored iteration.
Each test prints its figures before it asserts.
"""
import functools
import os

import numpy as np
import pytest
import torch

import antialias_cases as ac
import raster_cases as rc
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu
BAR = 4.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "antialias.npz"))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Per case, computed once and left unchanged: the inputs on the GPU, the kernels' rast layers and edge neighbours, and the
    restated decisions of both layers (CPU)."""
    from meshdiffusion_amd import render
    pc, faces, H, W = ac.case_inputs(case)
    nbr_np = ac.edge_neighbours_restated(faces.numpy(), pc.shape[1])
    pc_g, faces_g = pc.cuda(), faces.cuda()
    rast = render.rasterize(pc_g, faces_g, (H, W))
    nbr = render.edge_neighbours(faces_g, pc.shape[1])
    dec = [ac.pair_decisions(r.cpu(), pc, faces, torch.as_tensor(nbr_np)) for r in rast]
    return dict(pc=pc, faces=faces, pc_g=pc_g, faces_g=faces_g, rast=rast, nbr=nbr, nbr_np=nbr_np, dec=dec, H=H, W=W)


def _records(pairs):
    """The int32 records [B,H,W,2,4] -> (active, va, vb, p_first, w) on the CPU."""
    p = pairs.cpu()
    return p[..., 0] >= 0, p[..., 0].to(torch.int64), p[..., 1].to(torch.int64), p[..., 3] != 0, p[..., 2].contiguous().view(torch.float32)


def _meshes():
    tv, tf = ac.param_torus()
    sv, sf = rc.mesh("sphere")
    return {"tetrahedron": (torch.tensor([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]]), 4),
            "quad": (ac.small_mesh("quad")[1], 4), "fan3": (ac.small_mesh("fan3")[1], 5), "ptorus": (tf, tv.shape[0]),
            "sphere": (sf, sv.shape[0])}


@pytest.mark.parametrize("name", ("tetrahedron", "quad", "fan3", "ptorus", "sphere"))
def test_edge_neighbours_equal_the_restatement(hip_lib, name):
    from meshdiffusion_amd import render
    faces, n_verts = _meshes()[name]
    want = ac.edge_neighbours_restated(faces.numpy(), n_verts)
    got = render.edge_neighbours(faces.cuda(), n_verts)
    print(f"\n{name}: F {faces.shape[0]} edges without a neighbour {int((want < 0).sum())}")
    assert got.dtype == torch.int32 and got.shape == (faces.shape[0], 3)
    assert torch.equal(got.cpu(), torch.as_tensor(want))
    assert torch.equal(render.edge_neighbours(faces.cuda(), n_verts), got)
    if name == "tetrahedron":
        assert bool((got >= 0).all())
    if name == "quad":
        assert int((got < 0).sum()) == 4
    if name == "fan3":
        assert bool((got < 0).all())
    assert render.edge_neighbours(torch.zeros(0, 3, dtype=torch.int64).cuda(), 3).shape == (0, 3)


@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_pair_decisions_equal_the_restatement(hip_lib, case):
    from meshdiffusion_amd import render
    ref = _reference(case)
    assert torch.equal(ref["nbr"].cpu(), torch.as_tensor(ref["nbr_np"]))
    for layer in (0, 1):
        rast, dec = ref["rast"][layer], ref["dec"][layer]
        mask = (rast[..., 3:4] > 0).float()
        out, pairs = render.antialias(mask, rast, ref["pc_g"], ref["faces_g"], ref["nbr"], return_pairs=True)
        active, va, vb, p_first, w = _records(pairs)
        w32 = ac.pair_weights(ref["pc"], dec, torch.float32)
        cand = int((rast[:, :, :-1, 3] != rast[:, :, 1:, 3]).sum() + (rast[:, :-1, :, 3] != rast[:, 1:, :, 3]).sum())
        print(f"\n{ac.case_id(case)} layer {layer}: candidate pairs {cand} active {int(active.sum())} (restated {int(dec['active'].sum())}) "
              f"largest |w - restated fp32 w| {float((w - w32).abs().max()):.2e}")
        assert pairs.dtype == torch.int32 and pairs.shape == (*rast.shape[:3], 2, 4) and not out.requires_grad
        assert torch.equal(active, dec["active"])
        assert torch.equal(va, dec["va"]) and torch.equal(vb, dec["vb"])
        assert torch.equal(p_first & active, dec["p_first"])
        assert torch.equal((w < 0) & active, (w32 < 0) & dec["active"])           # the receiver
        assert torch.equal(w, w32)                                                  # fp32, every operation rounded on its own
        # away from the active pairs the image is untouched, and the mask stays in [0, 1]
        touched = torch.zeros(mask.shape[:3], dtype=torch.bool)
        touched |= active[..., 0] | active[..., 1]
        touched[:, :, 1:] |= active[:, :, :-1, 0]
        touched[:, 1:] |= active[:, :-1, :, 1]
        assert torch.equal(out.cpu()[~touched], mask.cpu()[~touched])
        assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    if case[0] != "sphere":
        assert int(ref["dec"][0]["active"].sum()) > 0
    else:                                                                           # near pixel-size triangles: almost all pairs exit early
        assert 0 < int(ref["dec"][0]["active"].sum()) < 0.1 * cand


@pytest.mark.parametrize("kind", ac.COLOURS)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_values_and_gradients_against_float64(hip_lib, gold, case, kind):
    from meshdiffusion_amd import render
    ref = _reference(case)
    cid = ac.case_id(case)
    nbr_cpu = torch.as_tensor(ref["nbr_np"])
    for layer in (0, 1):
        rast, dec = ref["rast"][layer], ref["dec"][layer]
        col = ac.case_colour(kind, rast[..., 3].cpu() > 0, int(gold["case/c_seed"]))
        G = ac.case_G(col.shape, int(gold["case/g_seed"]))
        v64, dc64, dp64 = ac.grads_restated(col, rast.cpu(), ref["pc"], ref["faces"], nbr_cpu, G, torch.float64, dec)
        runs = []
        for _ in range(2):
            c = col.cuda().requires_grad_(True)
            p = ref["pc_g"].clone().requires_grad_(True)
            out = render.antialias(c, rast, p, ref["faces_g"], ref["nbr"])
            assert out.grad_fn is not None and out.dtype == torch.float32 and out.shape == col.shape
            (out * G.cuda()).sum().backward()
            runs.append((out.detach(), c.grad, p.grad))
        for a, b in zip(*runs):
            assert torch.equal(a, b)                                                # no atomics: bit-identical runs
        out, dc, dp = runs[0]
        key = f"case/{cid}/L{layer}/{kind}"
        msg, ok = [], True
        for q, got, want in (("value", out, v64), ("dcolor", dc, dc64), ("dpos", dp, dp64)):
            err, unit = rc.rel_l2(got, want), float(gold[f"{key}/ref_err_{q}"])
            msg.append(f"{q} {err:.3e} / {unit:.3e} = {err / unit if unit > 0 else float(err > 0):.2f}")
            ok = ok and err <= BAR * unit
        print(f"\n{cid} layer {layer} {kind}: rel-L2 vs float64 / fp32 restatement's own: " + "  ".join(msg))
        assert dp.shape == ref["pc_g"].shape and bool(torch.isfinite(dp).all()) and not bool(dp[..., 2].any())
        on_edge = torch.zeros(ref["pc"].shape[:2], dtype=torch.bool)
        b = torch.nonzero(dec["active"])[:, 0]
        on_edge[b, dec["va"][dec["active"]]] = True
        on_edge[b, dec["vb"][dec["active"]]] = True
        assert not bool(dp.cpu()[~on_edge].any())
        if layer == 0 and case[0] in ("ptorus", "sphere", "wneg"):               # every vertex of quad and fan3 is on the silhouette
            assert bool((~on_edge).any()) and bool(on_edge.any())
        assert ok, (cid, layer, kind)


def test_no_faces_and_ids_above_the_face_count(hip_lib):
    from meshdiffusion_amd import render
    pc, faces, H, W = ac.case_inputs(ac.CASES[1])
    col = torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
    p = pc.cuda().requires_grad_(True)
    rast = torch.zeros(2, H, W, 4, device="cuda")
    out = render.antialias(col, rast, p, torch.zeros(0, 3, dtype=torch.int64).cuda())
    G = torch.randn(2, H, W, 3, generator=torch.Generator().manual_seed(5)).cuda()
    (out * G).sum().backward()
    assert torch.equal(out, col.detach()) and torch.equal(col.grad, G) and not bool(p.grad.any())
    # ids above F (never written by the rasteriser) make their pairs inactive and are never an index
    rast[..., 3] = torch.randint(faces.shape[0] + 1, 2 ** 24, (2, H, W), generator=torch.Generator().manual_seed(6)).float().cuda()
    rast[..., 2] = 0.5
    out, pairs = render.antialias(col.detach(), rast, pc.cuda(), faces.cuda(), return_pairs=True)
    assert torch.equal(out, col.detach()) and bool((pairs[..., 0] == -1).all())


def test_render_depth_with_alpha(hip_lib, gold):
    from meshdiffusion_amd import render
    case = ac.CASES[1]
    verts, faces = ac.param_torus()
    H, W = case[1:]
    mvp, campos = rc.cameras(rc.ANGLES, H, W)
    G = ac.case_G((2, mvp.shape[0], H, W, 1), int(gold["case/g_seed"]))
    grads = []
    for _ in range(2):
        v = verts.cuda().requires_grad_(True)
        out = render.render_depth(v, faces.cuda(), mvp.cuda(), campos.cuda(), (H, W), antialias=True)
        assert set(out) == {"depth", "depth_second", "mask", "mask_second", "rast", "rast_second", "rast_triangle_id", "alpha",
                            "alpha_second"}
        assert out["alpha"].grad_fn is not None and out["alpha_second"].grad_fn is not None
        ((out["alpha"] * G[0].cuda()).sum() + (out["alpha_second"] * G[1].cuda()).sum()).backward()
        grads.append(v.grad)
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().sum()) > 0
    plain = render.render_depth(verts.cuda(), faces.cuda(), mvp.cuda(), campos.cuda(), (H, W))
    assert "alpha" not in plain and torch.equal(plain["depth"], out["depth"].detach())
    # alpha equals the mask wherever no pair is active, and lies in [0, 1]
    ref = _reference(case)
    for layer, (a, m) in enumerate((("alpha", "mask"), ("alpha_second", "mask_second"))):
        assert torch.equal(out[m.replace("mask", "rast")], ref["rast"][layer])
        active = ref["dec"][layer]["active"]
        touched = active[..., 0] | active[..., 1]
        touched[:, :, 1:] |= active[:, :, :-1, 0]
        touched[:, 1:] |= active[:, :-1, :, 1]
        alpha = out[a].detach().cpu()
        assert alpha.shape == (2, H, W, 1) and torch.equal(alpha[~touched], out[m].cpu()[~touched])
        assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0 and bool((alpha != out[m].cpu()).any())
    # the gradient against the float64 chain through xfm_points
    v64 = verts.double().requires_grad_(True)
    a1, a2, _, _ = ac.alpha_restated(v64, faces, mvp, H, W, torch.float64, [r.cpu() for r in ref["rast"]])
    ((a1 * G[0]).sum() + (a2 * G[1]).sum()).backward()
    err, unit = rc.rel_l2(grads[0], v64.grad), float(gold[f"alpha/{ac.case_id(case)}/ref_err_dverts"])
    print(f"\nalpha {ac.case_id(case)}: d verts rel-L2 vs float64 {err:.3e}, fp32 restatement's own {unit:.3e}, ratio {err / unit:.2f}")
    tgt = render.make_targets(verts.cuda(), faces.cuda(), mvp.cuda(), campos.cuda(), (H, W), antialias=True)
    assert set(tgt) == {"depth", "depth_second", "mask_cont", "mvp", "campos", "resolution", "alpha", "alpha_second"}
    assert torch.equal(tgt["alpha"], out["alpha"].detach()) and not tgt["alpha"].requires_grad
    assert float(render.silhouette_loss(out, tgt).detach()) == 0.0
    assert err <= BAR * unit


def test_fit_to_views_with_the_alpha_term(hip_lib, gold):
    """fit_to_views(alpha_weight=1, return_terms=True) on the shipped 64 tet grid from a sphere of radius 0.9 to the torus: 4 views
    at 256 x 256, 21 iterations, no chamfer, no carve.  Bar: the depth and the alpha term at iterations 0, 10, 20 within
    4 x max(|fp32 - float64|, 1e-6 |float64|) of the float64 value of the restated loop."""
    from meshdiffusion_amd import render
    from meshdiffusion_amd.dmtet import DMTetGeometry
    geo = DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(rc.fit_initial_sdf(geo.verts))
        geo.deform.zero_()
    mvp, campos = rc.cameras(rc.FIT_ANGLES, ac.FIT_RES, ac.FIT_RES)
    tv, tf = rc.mesh("torus")
    plain = render.make_targets(tv.cuda(), tf.cuda(), mvp.cuda(), campos.cuda(), ac.FIT_RES)
    with pytest.raises(ValueError):
        render.fit_to_views(geo, plain, 1, alpha_weight=1.0)                        # needs alpha targets
    targets = render.make_targets(tv.cuda(), tf.cuda(), mvp.cuda(), campos.cuda(), ac.FIT_RES, antialias=True)
    terms = render.fit_to_views(geo, targets, ac.FIT_ITERS, lr=rc.FIT_LR, sdf_regularizer=rc.FIT_SDF_REGULARIZER, carve=False,
                                alpha_weight=ac.FIT_ALPHA_WEIGHT, return_terms=True)
    assert set(terms) == {"depth", "alpha"} and all(t.shape == (ac.FIT_ITERS,) and t.dtype == torch.float32 for t in terms.values())
    ok = True
    for name in ("depth", "alpha"):
        got = terms[name].double().cpu().numpy()[list(ac.FIT_STEPS)]
        l32, l64 = gold[f"fit/{name}32"], gold[f"fit/{name}64"]
        unit = np.maximum(np.abs(l32 - l64), 1e-6 * np.abs(l64))
        ratio = np.abs(got - l64) / unit
        print(f"\nfit: {name} term {got} float64 restated loop {l64} fp32 restated loop {l32} |gpu - f64| / unit {ratio}")
        ok = ok and bool((ratio <= BAR).all())
    print(f"float64 loop from radius {ac.FIT_SMALL_RADIUS}: final silhouette IoU with alpha_weight 0 / 1 {gold['fit/iou_small_start']}")
    assert ok


def test_fit_views_tool_with_alpha_weight(hip_lib, tmp_path):
    """tools/fit_views.py --alpha_weight 1 in this process: three iterations still write a dict that dicts_to_grids reads."""
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
               "--views_per_iter", "2", "--iters", "3", "--sphere_init", "0.9", "--points", "2000", "--alpha_weight", "1",
               "--out", out])
    d = torch.load(out, map_location="cpu", weights_only=False)
    n = rc.tet_grid()[0].shape[0]
    assert set(d) == {"sdf", "deform"} and d["sdf"].shape == (n,) and d["deform"].shape == (n, 3)
    written = mesh_export.dicts_to_grids(rc.tet_grid()[0], str(tmp_path / "fitted"), str(tmp_path / "grids"), 64, [0])
    assert len(written) == 1
    grid = torch.load(written[0], map_location="cpu", weights_only=False)
    assert tuple(grid.shape) == (4, 64, 64, 64) and bool(torch.isfinite(grid).all()) and bool(grid[0].any())
