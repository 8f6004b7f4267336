"""Host side of the mesh post-processing (csrc/meshpost.hip, meshdiffusion_amd/postprocess.py, the preview of
meshdiffusion_amd/render.py, the PNG writer of meshdiffusion_amd/mesh_export.py) without a GPU: the export tables, argument refusal,
the restatements of tests/meshpost_cases.py against each other and against hand-made answers, the light, the PNG round trip and the
recorded units.  Each test prints its figures before it asserts."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import interp_cases as ic
import meshpost_cases as mc
from conftest import GOLD, ROOT


def test_new_exports_are_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import _lib, build, mesh_export, postprocess, render
    header = open(os.path.join(ROOT, "include", "meshdiffusion_hip.h")).read()
    assert "meshpost.hip" in build.SOURCES
    assert _lib.MESHPOST_MAX_ROUNDS == mc.MAX_ROUNDS == 64 and "#define MD_MESHPOST_MAX_ROUNDS 64" in header
    assert _lib.MESH_COMPONENTS_WORKSPACE_BYTES == 16
    src = open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "meshpost.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "THE MESH POST-PROCESSING CONTRACT" in src
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*float", src) and "unsafeAtomicAdd" not in src
    for mod, names in ((postprocess, ("mesh_edges", "smooth", "components", "drop_floaters", "concat_meshes", "split_meshes", "postprocess")),
                       (render, ("sh9_from_latlong", "default_light", "preview_camera", "shade_diffuse", "render_preview")),
                       (mesh_export, ("save_png", "load_png"))):
        for name in names:
            assert callable(getattr(mod, name)), name


def test_new_exports_refuse_bad_arguments_without_a_gpu(hip_lib):
    nul, one, odd4, odd8, odd16 = C.c_void_p(0), C.c_void_p(64), C.c_void_p(66), C.c_void_p(68), C.c_void_p(72)
    two, three = C.c_void_p(128), C.c_void_p(192)

    def check(fn, ok, pointers, sizes, unsupported, misaligned):
        for k in pointers:
            a = list(ok); a[k] = nul
            assert fn(*a) == -1, (fn.__name__, k)
        for k in sizes:
            for bad in (0, -3):
                a = list(ok); a[k] = bad
                assert fn(*a) == -1, (fn.__name__, k, bad)
        for k, v in unsupported:
            a = list(ok); a[k] = v
            assert fn(*a) == -2, (fn.__name__, k, v)
        for k, p in misaligned:
            a = list(ok); a[k] = p
            assert fn(*a) == -1, (fn.__name__, k)

    # md_mesh_smooth(verts, ptr, adj, V, n_codes, steps, lam, mu, out, scratch, stream)
    fn = hip_lib.md_mesh_smooth
    ok = [one, one, one, 100, 600, 3, 0.5, float("nan"), two, three, nul]
    check(fn, ok, (0, 1, 2, 8, 9), (3, 4), ((3, 1 << 30), (3, 1 << 40), (4, 1 << 31)), ((0, odd4), (1, odd4), (2, odd4), (8, odd4), (9, odd4)))
    for k, bad in ((5, -1), (6, float("inf")), (6, float("nan")), (7, float("inf")), (7, -float("inf"))):
        a = list(ok); a[k] = bad
        assert fn(*a) == -1, (k, bad)
    for k, other in ((8, one), (9, one), (9, two)):                     # the input is never written: no aliasing
        a = list(ok); a[k] = other
        assert fn(*a) == -1, (k, "alias")
    # md_mesh_components(faces, V, F, label, comp_faces, workspace, rounds, stream)
    rounds = C.c_int32(7)
    ok = [one, 100, 300, one, one, one, C.byref(rounds), nul]
    check(hip_lib.md_mesh_components, ok, (0, 3, 4, 5), (1, 2), ((1, 1 << 31), (2, 1 << 30), (2, 1 << 40)),
          ((0, odd8), (3, odd4), (4, odd4), (5, odd4)))
    assert rounds.value == 0
    ok[6] = None                                                         # rounds is optional
    assert hip_lib.md_mesh_components(*[nul if k == 0 else a for k, a in enumerate(ok)]) == -1
    # md_shade_diffuse(rast, verts, faces, campos, sh, kd, B, V, F, H, W, out, stream)
    ok = [one, one, one, one, one, one, 2, 100, 300, 16, 16, one, nul]
    check(hip_lib.md_shade_diffuse, ok, (0, 1, 2, 3, 4, 5, 11), (6, 7, 8, 9, 10),
          ((6, 65), (7, 1 << 31), (8, 1 << 24), (9, 2049), (10, 2049)),
          ((0, odd16), (11, odd16), (2, odd8), (1, odd4), (3, odd4), (4, odd4), (5, odd4)))


def test_python_entry_points_refuse_cpu_tensors_and_bad_shapes():
    from meshdiffusion_amd import _lib, postprocess, render
    v, f = mc.mesh("quad")
    mvp, campos = render.preview_camera(0, 16)
    for call in (lambda: postprocess.mesh_edges(f, 4), lambda: postprocess.smooth(v, f), lambda: postprocess.components(f, 4),
                 lambda: postprocess.drop_floaters(v, f), lambda: postprocess.postprocess([(v, f)], smooth_steps=1),
                 lambda: render.shade_diffuse(torch.zeros(1, 4, 4, 4), v, f, campos, render.default_light(), render.PREVIEW_KD),
                 lambda: render.render_preview(v, f, mvp, campos, 16)):
        with pytest.raises(_lib.MeshDiffusionHipError):
            call()                                                       # CPU tensors: no fallback


def test_edge_table_and_smoothing_on_hand_made_answers():
    v, f = mc.mesh("quad")
    lo, hi, mult, ptr, adj = mc.edges_restated(f, 4)
    assert list(zip(lo, hi, mult)) == [(0, 1, 1), (0, 2, 2), (0, 3, 1), (1, 2, 1), (2, 3, 1)]
    assert ptr.tolist() == [0, 3, 5, 8, 10] and adj.tolist() == [3, 4, 7, 1, 5, 0, 3, 7, 1, 5]
    nb, n = mc.smoothing_rows(f, 4)
    assert n.tolist() == [2, 2, 2, 2] and nb[:, :2].tolist() == [[1, 3], [0, 2], [1, 3], [0, 2]]      # every vertex is on the boundary
    x = mc.smooth_restated(v, f, 1, 0.5, None, torch.float64)
    want = v.double() + 0.5 * ((v.double()[[1, 0, 1, 0]] + v.double()[[3, 2, 3, 2]]) / 2 - v.double())
    assert float((x - want).abs().max()) <= 1e-15
    assert torch.equal(mc.smooth_restated(v, f, 0, 0.5, None, torch.float32), v)
    # degen: the edge (1, 2) belongs to faces 0 and 3 (face 3 names 1 twice: its (1, 1) edge is dropped, (1, 2) counted twice)
    v, f = mc.mesh("degen")
    lo, hi, mult, ptr, adj = mc.edges_restated(f, 8)
    table = {(int(a), int(b)): int(m) for a, b, m in zip(lo, hi, mult)}
    print(f"\ndegen edges {table}")
    assert table == {(0, 1): 1, (0, 2): 2, (0, 3): 1, (1, 2): 3, (2, 3): 1, (5, 6): 1, (5, 7): 1, (6, 7): 1}
    nb, n = mc.smoothing_rows(f, 8)
    assert n.tolist() == [2, 1, 1, 2, 0, 2, 2, 2]
    for tag, steps, lam, mu in mc.SMOOTH_SETTINGS:
        x = mc.smooth_restated(v, f, steps, lam, mu, torch.float32)
        assert torch.equal(x[4], v[4]) and torch.equal(x[5:], v[5:])     # no row; three copies of one point average to it
    # Taubin does not shrink what plain smoothing shrinks
    v, f = mc.mesh("ptorus")
    r = [float(mc.smooth_restated(v, f, 10, 0.5, mu).norm() / v.norm()) for mu in (None, -0.53)]
    print(f"ptorus after 10 steps: |x| / |x0| plain {r[0]:.4f} Taubin {r[1]:.4f}")
    assert r[0] < 0.97 < r[1] < 1.03
    # the batched form equals the two meshes done alone
    pv, pf = mc.mesh("pair")
    both = mc.smooth_restated(pv, pf, 3, 0.5, None, torch.float32)
    a, b = (mc.smooth_restated(*mc.mesh(n), 3, 0.5, None, torch.float32) for n in ("ptorus", "fan40"))
    assert torch.equal(both, torch.cat([a, b]))


@pytest.mark.parametrize("name", mc.CASES)
def test_hook_and_compress_reaches_scipys_labels(name):
    v, f = mc.mesh(name)
    V = v.shape[0]
    label, cf = mc.components_restated(f, V)
    sim, rounds = mc.rounds_simulated(f, V)
    lo, hi, mult, _, _ = mc.edges_restated(f, V)
    sizes = np.bincount(label, minlength=V)
    print(f"\n{name}: V {V} F {f.shape[0]} components {int((label == np.arange(V)).sum())} largest {int(sizes.max())} vertices / "
          f"{int(cf.max())} faces, boundary edges {int((mult == 1).sum())}, synchronous rounds {rounds}")
    assert np.array_equal(sim, label) and rounds <= mc.MAX_ROUNDS
    assert bool((label <= np.arange(V)).all()) and np.array_equal(label[label], label) and int(cf.sum()) == f.shape[0]
    assert not cf[label != np.arange(V)].any()
    if name == "degen":
        assert label.tolist() == mc.DEGEN_LABELS and cf.tolist() == [3, 0, 0, 0, 0, 1, 0, 0]
    if name == "noise":
        assert (V, f.shape[0]) == (97737, 199256) and int((label == np.arange(V)).sum()) == 27
        assert int(sizes.max()) == 97540 and int((mult == 1).sum()) == 8262
    if name == "strip4096":
        assert rounds > 4                                                # the labelling needs several rounds on it
    if name == "pair":
        assert sorted(set(label.tolist())) == [0, 128]


def test_drop_floaters_restated_on_hand_made_answers():
    v, f = mc.mesh("degen")
    nv, nf, vmap, keep = mc.drop_floaters_restated(v, f)                 # defaults: only the unreferenced vertex goes
    assert vmap.tolist() == [0, 1, 2, 3, -1, 4, 5, 6] and keep.all() and nf.tolist() == [[0, 1, 2], [0, 2, 3], [4, 5, 6], [1, 1, 2]]
    nv, nf, vmap, keep = mc.drop_floaters_restated(v, f, keep_largest=True)
    assert vmap.tolist() == [0, 1, 2, 3, -1, -1, -1, -1] and keep.tolist() == [True, True, False, True] and nv.shape == (4, 3)
    nv, nf, vmap, keep = mc.drop_floaters_restated(v, f, min_faces=4)
    assert nv.shape == (0, 3) and nf.shape == (0, 3) and not keep.any()
    nv, nf, vmap, keep = mc.drop_floaters_restated(v, f, min_fraction=0.34)      # ceil(0.34 * 3) = 2 > 1
    assert keep.tolist() == [True, True, False, True]
    pv, pf = mc.mesh("pair")
    nv, nf, vmap, keep = mc.drop_floaters_restated(pv, pf, keep_largest=True)    # as one mesh: the torus alone
    assert nv.shape[0] == 128 and int(keep.sum()) == 256
    nv, nf, vmap, keep = mc.drop_floaters_restated(pv, pf, keep_largest=True, vert_mesh=mc.vert_mesh("pair"))
    assert nv.shape[0] == 169 and keep.all()                                    # one component per mesh survives
    v, f = mc.mesh("noise")
    nv, nf, vmap, keep = mc.drop_floaters_restated(v, f, min_fraction=0.01)
    left = len(np.unique(mc.components_restated(nf, nv.shape[0])[0]))
    print(f"\nnoise at min_fraction 0.01: {left} of 27 components left, {nv.shape[0]} vertices {nf.shape[0]} faces")
    assert left == 1 and nv.shape[0] == 97540


def test_shading_restatement_properties():
    verts, faces, mvp, campos, pc, H, W, rast = mc.shade_inputs(("quad", 16, 16))
    white = torch.zeros(9, 3)
    white[0] = 1 / 0.282095
    kd = torch.tensor([0.75, 0.3, 0.6])
    out, gv, cov = mc.shade_restated(rast, verts, faces, campos, white, kd, torch.float64)
    print(f"\nquad: covered {int(cov.sum())}, geo . view per view {[float(gv[b][cov[b]].mean()) for b in range(2)]}")
    assert float((out[..., :3][cov] - kd.double()).abs().max()) <= 1e-7 and bool((out[..., 3][cov] == 1).all())
    assert not bool(out[~cov].any())
    assert bool((gv[0][cov[0]] > 0).all()) and bool((gv[1][cov[1]] < 0).all())       # front in view 0, behind in view 1
    sh, kd = mc.case_light("random")
    a = mc.shade_restated(rast, verts, faces, campos, sh, kd)[0]
    rast_f = rast.clone()                                                # two-sided: the winding does not matter
    rast_f[..., 0], rast_f[..., 1] = rast[..., 0], (1 - rast[..., 0]) - rast[..., 1]
    assert float((a - mc.shade_restated(rast_f, verts, faces[:, [0, 2, 1]], campos, sh, kd)[0]).abs().max()) <= 1e-6
    big = rast.clone()
    big[..., 3] = torch.where(cov, torch.full_like(big[..., 3], 3.0), big[..., 3])     # an id above F is never an index
    assert not bool(mc.shade_restated(big, verts, faces, campos, sh, kd)[0].any())


def test_sh9_from_latlong_white_and_smooth_environments():
    from meshdiffusion_amd import render
    h, w = mc.ENV_RES
    n = mc.seeded_normals(200)
    kd = np.array(render.PREVIEW_KD)
    sh = render.sh9_from_latlong(np.ones((h, w, 3)))
    assert sh.shape == (9, 3) and sh.dtype == np.float32
    e = kd * mc.irradiance_sh(sh, n)
    print(f"\nwhite {h}x{w}: max |kd e - kd| {np.abs(e - kd).max():.2e}; L0 {sh[0, 0]:.6f} largest other coefficient {np.abs(sh[1:]).max():.2e}")
    assert np.abs(e - kd).max() <= 2e-4
    env = mc.smooth_env()
    sh = render.sh9_from_latlong(torch.as_tensor(env))
    assert np.abs(sh - mc.sh9_restated(env)).max() <= 1e-6
    a, b = mc.irradiance_sh(sh, n), mc.irradiance_brute(env, n)
    print(f"smooth environment: max |SH - brute force| {np.abs(a - b).max():.2e} over a range {b.min():.2f}-{b.max():.2f}")
    assert np.abs(a - b).max() <= 1e-4
    light = render.default_light()
    assert light.shape == (9, 3) and light.dtype == np.float32 and np.array_equal(light, render.default_light())
    d = render.latlong_directions(h, w)[0]
    assert np.allclose(d, mc.latlong_restated(h, w)[0]) and np.abs(light - mc.sh9_restated(render.default_sky(d))).max() <= 1e-6
    lit = mc.irradiance_sh(light, n)
    print(f"default light: irradiance / pi over the normals {lit.min():.3f}-{lit.max():.3f}")
    assert lit.min() > 0.1 and lit.max() < 1.5
    with pytest.raises(ValueError):
        render.sh9_from_latlong(np.ones((4, 8)))


def test_preview_camera_is_rotate_scene():
    from meshdiffusion_amd import render
    import raster_cases as rc
    for ind in (0, 7, 25):
        mvp, campos = render.preview_camera(ind, 64)
        want_mvp, want_cam = rc.camera((ind / 50) * np.pi * 2, 64, 64)
        assert mvp.shape == (1, 4, 4) and campos.shape == (1, 3) and mvp.dtype == torch.float32
        assert float((mvp[0] - want_mvp).abs().max()) <= 1e-6 and float((campos[0] - want_cam).abs().max()) <= 1e-6
        assert abs(float(campos.norm()) - 3.0) <= 1e-5
    mvp, _ = render.preview_camera(0, (32, 64))                                    # aspect W / H
    mv = render.translate(0, 0, -3.0) @ (render.rotate_x(-0.4) @ render.rotate_y(0.0))
    want = torch.tensor(rc.perspective64(np.deg2rad(45.0), 2.0, 0.1, 1000.0), dtype=torch.float32) @ mv
    assert float((mvp[0] - want).abs().max()) <= 1e-6


def test_png_round_trip(tmp_path):
    from meshdiffusion_amd import mesh_export
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    mesh_export.save_png(path, img)
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    assert np.array_equal(mesh_export.load_png(path), img)
    x = rng.random((9, 5, 3)).astype(np.float32)
    x[0, 0] = (-0.2, 1.7, 0.5)
    mesh_export.save_png(path, torch.as_tensor(x))
    assert np.array_equal(mesh_export.load_png(path), np.clip(np.rint(x.astype(np.float64) * 255), 0, 255).astype(np.uint8))
    with pytest.raises(ValueError):
        mesh_export.save_png(path, np.zeros((4, 4)))
    Image = pytest.importorskip("PIL.Image")                            # the cross-check only
    mesh_export.save_png(path, img)
    assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img)
    Image.fromarray(img).save(path)                                      # a foreign writer's filters
    assert np.array_equal(mesh_export.load_png(path), img)


def test_fixture_is_small_and_holds_every_unit():
    gold = np.load(os.path.join(GOLD, "meshpost.npz"))
    assert os.path.getsize(os.path.join(GOLD, "meshpost.npz")) < 64 * 1024
    assert all(gold[k].size == 1 for k in gold.files)
    for name in mc.CASES:
        for tag, *_ in mc.SMOOTH_SETTINGS:
            assert 0 < float(gold[f"smooth/{name}/{tag}/ref_err"]) < 1e-6, (name, tag)
    for case in mc.SHADE_CASES:
        for light in mc.LIGHTS:
            assert 0 < float(gold[f"shade/{ic.case_id(case)}/{light}/ref_err"]) < 1e-6, (case, light)
        assert float(gold[f"shade/{ic.case_id(case)}/flip_margin"]) >= ic.FLIP_MARGIN
    assert len(gold.files) == len(mc.CASES) * len(mc.SMOOTH_SETTINGS) + len(mc.SHADE_CASES) * (len(mc.LIGHTS) + 1)


def test_synthetic_samples_hold_a_floater():
    s = mc.sphere_and_blob_samples()
    assert s.shape == (2, 4, 64, 64, 64) and s.dtype == np.float32 and set(np.unique(s[:, 0])) == {-1.0, 1.0} and not s[:, 1:].any()
    assert math.isclose(float((s[0, 0] < 0).mean()), 4 / 3 * math.pi * (0.25 ** 3 + 0.05 ** 3), rel_tol=0.05)
