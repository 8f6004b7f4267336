"""Attribute interpolation, the barycentric backward, the deterministic vertex normals and the `bsdf == 'normal'` renderer on the
GPU (csrc/interp.hip, meshdiffusion_amd/render.py, meshdiffusion_amd/dmtet.py) against the restatements of the interpolation
contract in tests/interp_cases.py, fed the kernels' own `rast`.

Bars, none fitted to what the kernels give:
  value, d attr, d rast, d pos_clip, d verts, normals   rel-L2 against the float64 restatement <= 4 x the fp32 torch restatement's
                    OWN rel-L2 distance from float64 for that case, layer and quantity, recorded in tests/golden/interp.npz by
                    tools/gen_golden_interp.py (the margin of tests/test_gpu_antialias.py); a unit of 0 demands an exact result.
  fitting run       4 x max(|fp32 loop - float64 loop|, 1e-6 |float64|) of the restated loop at each stored iteration.
Each test prints its figures before it asserts.
"""
import functools
import os

import numpy as np
import pytest
import torch

import antialias_cases as ac
import interp_cases as ic
import raster_cases as rc
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu
BAR = 4.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "interp.npz"))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Per case, computed once and left unchanged: the inputs on both devices and the kernels' own rast layers."""
    from meshdiffusion_amd import render
    verts, faces, mvp, campos, pc, H, W = ic.case_inputs(case)
    rast = render.rasterize(pc.cuda(), faces.cuda(), (H, W))
    return dict(verts=verts, faces=faces, mvp=mvp, campos=campos, pc=pc, H=H, W=W, rast=rast, rast_cpu=[r.cpu() for r in rast])


def _within(err, unit):
    return err <= BAR * unit if unit > 0 else err == 0.0


def _ratio(err, unit):
    return err / unit if unit > 0 else float(err > 0)


def _err(got, want):
    return rc.rel_l2(got, want) if float(want.abs().max()) > 0 else float(got.double().abs().max())


@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_interpolate_values_and_gradients_against_float64(hip_lib, gold, case):
    from meshdiffusion_amd import render
    ref = _reference(case)
    cid = ic.case_id(case)
    B, H, W, V, F = ref["pc"].shape[0], ref["H"], ref["W"], ref["verts"].shape[0], ref["faces"].shape[0]
    ok, lines = True, []
    for layer in (0, 1):
        rast, rast_cpu = ref["rast"][layer], ref["rast_cpu"][layer]
        cov = ic.covered(rast_cpu, F)
        for name, tri, N, C, Ba in ic.attr_cases(V, F, ref["faces"], B):
            attr = ic.case_attr(N, C, Ba, int(gold["case/a_seed"]))
            G = ic.case_G((B, H, W, C), int(gold["case/g_seed"]))
            want = ic.interpolate_grads_restated(attr, rast_cpu, tri, G, torch.float64)
            runs = []
            for _ in range(2):
                a = attr.cuda().requires_grad_(True)
                r = rast.clone().requires_grad_(True)
                out = render.interpolate(a if Ba > 1 or C != 3 else a[0], r, tri.cuda(), rast_grad=True)
                assert out.shape == (B, H, W, C) and out.dtype == torch.float32 and out.grad_fn is not None
                (out * G.cuda()).sum().backward()
                runs.append((out.detach(), a.grad, r.grad))
            for x, y in zip(*runs):
                assert torch.equal(x, y)                                            # no atomics: bit-identical runs
            out, da, dr = runs[0]
            assert not bool(out.cpu()[~cov].any()) and not bool(dr.cpu()[~cov].any()) and not bool(dr[..., 2:].any())
            msg = []
            for q, got, w64 in zip(("value", "dattr", "drast"), (out, da, dr), want):
                err, unit = _err(got.cpu(), w64), float(gold[f"case/{cid}/L{layer}/{name}/ref_err_{q}"])
                msg.append(f"{q} {err:.2e}/{unit:.2e}={_ratio(err, unit):.2f}")
                ok = ok and _within(err, unit)
            lines.append(f"L{layer} {name}: " + " ".join(msg))
            # without rast_grad, rast gets no gradient
            r = rast.clone().requires_grad_(True)
            plain = render.interpolate(attr.cuda().requires_grad_(True), r, tri.cuda())
            plain.sum().backward()
            assert r.grad is None and torch.equal(plain.detach(), out)
    print(f"\n{cid}: rel-L2 vs float64 / fp32 restatement's own = ratio\n  " + "\n  ".join(lines))
    assert ok, cid


def test_interpolate_ids_above_the_face_count_and_no_faces(hip_lib):
    from meshdiffusion_amd import render
    ref = _reference(ic.CASES[1])
    B, H, W, F, V = 2, ref["H"], ref["W"], ref["faces"].shape[0], ref["verts"].shape[0]
    rast = torch.rand(B, H, W, 4, generator=torch.Generator().manual_seed(3))
    rast[..., 3] = torch.randint(F + 1, 2 ** 24, (B, H, W), generator=torch.Generator().manual_seed(6)).float()
    attr = torch.rand(V, 3).cuda().requires_grad_(True)
    r = rast.cuda().requires_grad_(True)
    out = render.interpolate(attr, r, ref["faces"].cuda(), rast_grad=True)
    out.sum().backward()
    assert not bool(out.any()) and not bool(attr.grad.any()) and not bool(r.grad.any())
    # F = 0
    attr = torch.rand(V, 3).cuda().requires_grad_(True)
    r = ref["rast"][0].clone().requires_grad_(True)
    out = render.interpolate(attr, r, torch.zeros(0, 3, dtype=torch.int64).cuda(), rast_grad=True)
    out.sum().backward()
    assert out.shape == (B, H, W, 3) and not bool(out.any()) and not bool(attr.grad.any()) and not bool(r.grad.any())


@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_interpolated_position_gives_the_depth_of_render_depth(hip_lib, gold, case):
    from meshdiffusion_amd import render
    ref = _reference(case)
    cid = ic.case_id(case)
    v, f, mvp, campos = ref["verts"].cuda(), ref["faces"].cuda(), ref["mvp"].cuda(), ref["campos"].cuda()
    buf = render.render_depth(v, f, mvp, campos, (ref["H"], ref["W"]))
    ok = True
    for layer, key in enumerate(("depth", "depth_second")):
        rast = ref["rast"][layer]
        assert torch.equal(buf["rast" if layer == 0 else "rast_second"], rast)
        pos = render.interpolate(v, rast, f)
        cov = rast[..., 3] > 0
        d = torch.where(cov, (pos - campos[:, None, None, :]).norm(dim=-1), torch.zeros_like(cov, dtype=torch.float32))
        want = ic.chain_depth_restated(ref["verts"], ref["faces"], ref["mvp"], ref["campos"], ref["rast_cpu"][layer], torch.float64)
        own = torch.where(cov, buf[key][..., 0], torch.zeros_like(d))
        unit = float(gold[f"case/{cid}/L{layer}/ref_err_depth"])
        e1, e2 = _err(d.cpu(), want), _err(own.cpu(), want)
        print(f"\n{cid} layer {layer}: depth rel-L2 vs float64: interpolate + distance {e1:.2e} render_depth {e2:.2e} unit {unit:.2e}")
        ok = ok and _within(e1, unit) and _within(e2, unit)
    assert ok


@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_rasterize_with_grad(hip_lib, gold, case):
    from meshdiffusion_amd import render
    ref = _reference(case)
    cid = ic.case_id(case)
    B, H, W, F = ref["pc"].shape[0], ref["H"], ref["W"], ref["faces"].shape[0]
    f = ref["faces"].cuda()
    G4 = ic.case_G((B, H, W, 4), int(gold["case/g_seed"]) + 1)
    ok = True
    for layer in (0, 1):
        runs = []
        for _ in range(2):
            p = ref["pc"].cuda().requires_grad_(True)
            layers = render.rasterize(p, f, (H, W), grad=True)
            assert len(layers) == 2 and all(x.grad_fn is not None for x in layers)
            assert torch.equal(layers[0].detach(), ref["rast"][0]) and torch.equal(layers[1].detach(), ref["rast"][1])
            (layers[layer] * G4.cuda()).sum().backward()
            runs.append(p.grad)
        assert torch.equal(runs[0], runs[1])
        dp = runs[0].cpu()
        want = ic.bary_grad_restated(ref["pc"], ref["faces"], ref["rast_cpu"][layer], G4, torch.float64)
        err, unit = _err(dp, want), float(gold[f"case/{cid}/L{layer}/ref_err_dpos"])
        print(f"\n{cid} layer {layer}: d pos_clip rel-L2 vs float64 {err:.3e}, fp32 restatement's own {unit:.3e}, ratio {_ratio(err, unit):.2f}")
        assert dp.shape == ref["pc"].shape and bool(torch.isfinite(dp).all()) and not bool(dp[..., 2].any())
        seen = torch.zeros(ref["pc"].shape[:2], dtype=torch.bool)
        ids = ref["rast_cpu"][layer][..., 3].long()
        for b in range(B):
            vis = ids[b][ids[b] > 0] - 1
            seen[b, ref["faces"][vis].reshape(-1)] = True
        assert not bool(dp[~seen].any())                                            # vertices of no visible face: exactly zero
        ok = ok and _within(err, unit)
    assert not render.rasterize(ref["pc"].cuda().requires_grad_(True), f, (H, W))[0].requires_grad     # the default: detached
    assert ok


@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_chain_agrees_with_the_backward_of_render_depth(hip_lib, gold, case):
    """rasterize(grad=True) -> interpolate(verts, rast_grad=True) -> distance, against render_depth's own fused backward for the
    same G: both lie within 4 units of float64, so they lie within the sum of both bars of each other."""
    from meshdiffusion_amd import render
    ref = _reference(case)
    cid = ic.case_id(case)
    B, H, W = ref["pc"].shape[0], ref["H"], ref["W"]
    f, mvp, campos = ref["faces"].cuda(), ref["mvp"].cuda(), ref["campos"].cuda()
    G = ic.case_G((B, 2, H, W), int(gold["case/g_seed"]) + 2)
    v = ref["verts"].cuda().requires_grad_(True)
    layers = render.rasterize(render.xfm_points(v[None], mvp), f, (H, W), grad=True)
    loss = 0.0
    for k, r in enumerate(layers):
        pos = render.interpolate(v, r, f, rast_grad=True)
        cov = r.detach()[..., 3] > 0
        d = torch.where(cov[..., None], pos - campos[:, None, None, :], torch.ones_like(pos))
        loss = loss + (torch.where(cov, torch.sqrt((d * d).sum(-1)), torch.zeros_like(d[..., 0])) * G[:, k].cuda()).sum()
    loss.backward()
    v2 = ref["verts"].cuda().requires_grad_(True)
    buf = render.render_depth(v2, f, mvp, campos, (H, W))
    cov = [buf["mask"][..., 0], buf["mask_second"][..., 0]]
    ((buf["depth"][..., 0] * cov[0] * G[:, 0].cuda()).sum() + (buf["depth_second"][..., 0] * cov[1] * G[:, 1].cuda()).sum()).backward()
    ids = torch.stack([ref["rast_cpu"][0][..., 3], ref["rast_cpu"][1][..., 3]], 1).to(torch.int64)
    Gm = G * (ids > 0)
    want = rc.grad_restated(ref["verts"], ref["faces"], ref["mvp"], ref["campos"], ids, Gm, torch.float64)
    unit = float(gold[f"case/{cid}/ref_err_chain_dverts"])
    e1, e2, e12 = _err(v.grad.cpu(), want), _err(v2.grad.cpu(), want), float((v.grad - v2.grad).double().norm() / want.norm())
    print(f"\n{cid}: d verts rel-L2 vs float64: chain {e1:.3e} render_depth {e2:.3e}; chain vs render_depth {e12:.3e}; unit {unit:.3e}")
    assert _within(e1, unit) and _within(e2, unit) and e12 <= 2 * BAR * unit


@pytest.mark.parametrize("name", sorted({c[0] for c in ic.CASES}))
def test_vertex_normals(hip_lib, gold, name):
    from meshdiffusion_amd import dmtet
    verts, faces = ic.mesh(name)
    G = ic.case_G(verts.shape, int(gold["case/g_seed"]) + 3)
    n64, g64 = ic.vertex_normals_grads_restated(verts, faces, G, torch.float64)
    _, fn64, replaced = ic.vertex_normals_restated(verts, faces, torch.float64)
    runs = []
    for _ in range(2):
        v = verts.cuda().requires_grad_(True)
        v_nrm, f_nrm = dmtet.vertex_normals(v, faces.cuda())
        assert v_nrm.grad_fn is not None and f_nrm.grad_fn is not None and v_nrm.shape == verts.shape
        (v_nrm * G.cuda()).sum().backward()
        runs.append((v_nrm.detach(), v.grad, f_nrm.detach()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    n, g, fn = (x.cpu() for x in runs[0])
    e_n, e_g = _err(n, n64), _err(g, g64)
    u_n, u_g = float(gold[f"normals/{name}/ref_err_value"]), float(gold[f"normals/{name}/ref_err_dverts"])
    print(f"\nnormals {name}: V {verts.shape[0]} F {faces.shape[0]} replaced {int(replaced.sum())}  rel-L2 vs float64 / unit: value "
          f"{e_n:.2e}/{u_n:.2e}={_ratio(e_n, u_n):.2f} d verts {e_g:.2e}/{u_g:.2e}={_ratio(e_g, u_g):.2f} f_nrm {rc.rel_l2(fn, fn64):.2e}")
    assert float((n.norm(dim=1) - 1).abs().max()) <= 1e-5 and rc.rel_l2(fn, fn64) <= 1e-5
    up = torch.tensor([0.0, 0.0, 1.0])
    assert torch.equal(n[replaced], up.expand(int(replaced.sum()), 3))
    if name == "degen":
        assert replaced.tolist() == [False] * 4 + [True] * 4 and not bool(g[4:].any())
    if name == "fan40":
        assert int((faces == 0).sum()) == ic.FAN and bool(g[0].any()) and not bool(replaced.any())
    assert _within(e_n, u_n) and _within(e_g, u_g)


def test_get_mesh_with_normals_grad(hip_lib):
    from meshdiffusion_amd.dmtet import DMTetGeometry
    geo = DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(rc.fit_initial_sdf(geo.verts))
    plain, attached = geo.getMesh(), geo.getMesh(normals_grad=True)
    assert plain.v_nrm.grad_fn is None and not plain.v_nrm.requires_grad
    assert attached.v_nrm.grad_fn is not None and attached.v_nrm.shape == plain.v_nrm.shape
    err = float((attached.v_nrm.detach() - plain.v_nrm).abs().max())
    print(f"\ngetMesh: V {plain.v_pos.shape[0]} largest |deterministic - atomic normal| {err:.2e}")
    assert float((attached.v_nrm.detach().norm(dim=1) - 1).abs().max()) <= 1e-5     # the summation orders differ: no bar on err
    attached.v_nrm[:, 0].sum().backward()
    assert bool(geo.sdf.grad.any()) and bool(torch.isfinite(geo.sdf.grad).all())


BUFFER_KEYS = {"depth", "depth_second", "mask", "mask_second", "rast", "rast_second", "rast_triangle_id", "alpha", "alpha_second",
               "pos", "geo_normal", "normal", "shaded", "pos_second", "geo_normal_second", "normal_second", "shaded_second"}


@pytest.mark.parametrize("case", ic.BUFFER_CASES, ids=ic.case_id)
def test_render_buffers(hip_lib, gold, case):
    from meshdiffusion_amd import render
    ref = _reference(case)
    cid = ic.case_id(case)
    H, W = ref["H"], ref["W"]
    f, mvp, campos = ref["faces"].cuda(), ref["mvp"].cuda(), ref["campos"].cuda()
    nbr = torch.as_tensor(ac.edge_neighbours_restated(ref["faces"].numpy(), ref["verts"].shape[0]))
    dec = [ac.pair_decisions(r, ref["pc"], ref["faces"], nbr) for r in ref["rast_cpu"]]
    with torch.no_grad():
        b64 = ic.buffers_restated(ref["verts"], ref["faces"], ref["mvp"], ref["campos"], ref["rast_cpu"], torch.float64, dec=dec)
    G = ic.buffer_G(b64, int(gold["case/g_seed"]) + 10)
    grads = []
    for _ in range(2):
        v = ref["verts"].cuda().requires_grad_(True)
        buf = render.render_buffers(v, f, mvp, campos, (H, W))
        sum((buf[k] * G[k].cuda()).sum() for k in ic.GRAD_KEYS).backward()
        grads.append(v.grad)
    assert torch.equal(grads[0], grads[1])
    assert set(buf) == BUFFER_KEYS
    base = render.render_depth(ref["verts"].cuda(), f, mvp, campos, (H, W), antialias=True)
    for k, x in base.items():
        assert torch.equal(buf[k].detach(), x) if torch.is_tensor(x) else buf[k] is None, k
    want = ic.buffers_dverts_restated(ref["verts"], ref["faces"], ref["mvp"], ref["campos"], ref["rast_cpu"], G, torch.float64, dec)
    err, unit = _err(grads[0].cpu(), want), float(gold[f"buffers/{cid}/ref_err_dverts"])
    vals = {k: rc.rel_l2(buf[k].detach().cpu(), b64[k]) for k in ic.GRAD_KEYS + ("geo_normal", "geo_normal_second")}
    print(f"\nbuffers {cid}: kink pixels {[int(b64['kink' + t].sum()) for t in ('', '_second')]} values rel-L2 vs float64 "
          + " ".join(f"{k} {e:.1e}" for k, e in vals.items())
          + f"\n  d verts rel-L2 vs float64 {err:.3e}, fp32 restatement's own {unit:.3e}, ratio {_ratio(err, unit):.2f}")
    for tail, bg in (("", 20.0), ("_second", -1.0)):
        cov = (buf["mask" + tail] > 0)[..., 0]
        assert torch.equal(buf["shaded" + tail][..., 3:].detach(), buf["alpha" + tail].detach())
        assert bool((buf["pos" + tail].detach()[~cov] == bg).all())
        for k in ("normal", "geo_normal"):
            assert not bool(buf[k + tail].detach()[~cov].any())
        assert float(buf["normal" + tail].detach().norm(dim=-1).max()) <= 1 + 1e-5
        assert buf["shaded" + tail].shape == (2, H, W, 4) and buf["normal" + tail].shape == (2, H, W, 3)
    assert all(e <= 1e-5 for e in vals.values()), vals
    tgt = render.make_targets(ref["verts"].cuda(), f, mvp, campos, (H, W), shaded=True)
    assert set(tgt) == {"depth", "depth_second", "mask_cont", "mvp", "campos", "resolution", "alpha", "alpha_second", "img", "img_second"}
    assert torch.equal(tgt["img"], buf["shaded"].detach()) and not tgt["img"].requires_grad
    assert float(render.color_loss(buf, tgt).detach()) == 0.0 and float(render.silhouette_loss(buf, tgt).detach()) == 0.0
    assert _within(err, unit)


def _fit_geometry():
    from meshdiffusion_amd.dmtet import DMTetGeometry
    geo = DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(rc.fit_initial_sdf(geo.verts))
        geo.deform.zero_()
    return geo


def test_fit_to_views_with_the_colour_term(hip_lib, gold):
    """fit_to_views(color_weight=1, alpha_weight=1, return_terms=True) on the shipped 64 tet grid from a sphere of radius 0.9 to
    the torus: 4 views at 64 x 64, 21 iterations, no chamfer, no carve.  Bar: the three terms at iterations 0, 10, 20 within
    4 x max(|fp32 - float64|, 1e-6 |float64|) of the float64 value of the restated loop."""
    from meshdiffusion_amd import render
    mvp, campos = rc.cameras(rc.FIT_ANGLES, ic.FIT_RES, ic.FIT_RES)
    tv, tf = rc.mesh("torus")
    plain = render.make_targets(tv.cuda(), tf.cuda(), mvp.cuda(), campos.cuda(), ic.FIT_RES, antialias=True)
    with pytest.raises(ValueError):
        render.fit_to_views(_fit_geometry(), plain, 1, color_weight=1.0)            # needs img targets
    targets = render.make_targets(tv.cuda(), tf.cuda(), mvp.cuda(), campos.cuda(), ic.FIT_RES, shaded=True)
    kw = dict(lr=rc.FIT_LR, sdf_regularizer=rc.FIT_SDF_REGULARIZER, carve=False, alpha_weight=ic.FIT_ALPHA_WEIGHT, return_terms=True)
    terms = render.fit_to_views(_fit_geometry(), targets, ic.FIT_ITERS, color_weight=ic.FIT_COLOR_WEIGHT, **kw)
    assert set(terms) == {"depth", "alpha", "color"} and all(t.shape == (ic.FIT_ITERS,) and t.dtype == torch.float32 for t in terms.values())
    ok = True
    for name in ("depth", "alpha", "color"):
        got = terms[name].double().cpu().numpy()[list(ic.FIT_STEPS)]
        l32, l64 = gold[f"fit/{name}32"], gold[f"fit/{name}64"]
        unit = np.maximum(np.abs(l32 - l64), 1e-6 * np.abs(l64))
        ratio = np.abs(got - l64) / unit
        print(f"\nfit: {name} term {got} float64 restated loop {l64} fp32 restated loop {l32} |gpu - f64| / unit {ratio}")
        ok = ok and bool((ratio <= BAR).all())
    # color_weight = 0: the loop and its numbers are those of a call that never mentions the keyword
    a = render.fit_to_views(_fit_geometry(), targets, 5, color_weight=0.0, **kw)
    b = render.fit_to_views(_fit_geometry(), targets, 5, **kw)
    assert set(a) == {"depth", "alpha"} and torch.equal(a["depth"], b["depth"]) and torch.equal(a["alpha"], b["alpha"])
    assert ok


def test_fit_views_tool_with_color_weight(hip_lib, tmp_path):
    """tools/fit_views.py --color_weight 1 --dump_normals in this process: three iterations write a dict that dicts_to_grids
    reads, and the final shaded views as finite .npy files."""
    import importlib.util
    from meshdiffusion_amd import mesh_export
    spec = importlib.util.spec_from_file_location("fit_views", os.path.join(ROOT, "tools", "fit_views.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tv, tf = rc.mesh("torus")
    obj = str(tmp_path / "torus.obj")
    mesh_export.save_obj(obj, tv, tf)
    out = str(tmp_path / "fitted" / "dmt_dict_00000.pt")
    dump = str(tmp_path / "normals")
    tool.main(["--obj", obj, "--tet_path", os.path.join(GOLD, "64_tets_cropped.npz"), "--views", "4", "--res", "32",
               "--views_per_iter", "2", "--iters", "3", "--sphere_init", "0.9", "--color_weight", "1", "--dump_normals", dump,
               "--out", out])
    d = torch.load(out, map_location="cpu", weights_only=False)
    n = rc.tet_grid()[0].shape[0]
    assert set(d) == {"sdf", "deform"} and d["sdf"].shape == (n,) and d["deform"].shape == (n, 3)
    written = mesh_export.dicts_to_grids(rc.tet_grid()[0], str(tmp_path / "fitted"), str(tmp_path / "grids"), 64, [0])
    assert len(written) == 1
    views = sorted(os.listdir(dump))
    assert len(views) == 4 and all(x.endswith(".npy") for x in views)
    for x in views:
        img = np.load(os.path.join(dump, x))
        assert img.shape == (32, 32, 4) and img.dtype == np.float32 and np.isfinite(img).all()
    assert any(np.load(os.path.join(dump, x))[..., 3].any() for x in views)
