"""Textures without a GPU (meshdiffusion_amd/texture.py, csrc/texture.hip): the numpy restatement of the texture contract against
torch's grid_sample and its autograd, the wrap mode against a tiled texture, `face_atlas` under the CPU rasteriser of
tests/raster_cases.py, the argument refusal of every new export, and the textured `.obj` round trip."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import texture_cases as tc
from conftest import GOLD, ROOT


def _grid_sample(tex, uv):
    """float64 tensors: tex [B,Ht,Wt,C], uv [B,H,W,2] -> [B,H,W,C] by torch (border padding = clamped indices)."""
    out = torch.nn.functional.grid_sample(tex.permute(0, 3, 1, 2), uv * 2 - 1, mode="bilinear", padding_mode="border", align_corners=False)
    return out.permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", [((5, 3), 3, 2, (7, 5)), ((1, 5), 1, 1, (4, 9)), ((16, 16), 4, 3, (17, 33)), ((1, 1), 2, 2, (3, 3))])
def test_clamp_restatement_equals_grid_sample_and_its_autograd(shape):
    (Ht, Wt), Cc, B, (H, W) = shape
    rng = np.random.default_rng(5)
    tex = rng.standard_normal((B, Ht, Wt, Cc)).astype(np.float32)
    uv = rng.uniform(-0.5, 1.5, (B, H, W, 2)).astype(np.float32)
    G = rng.standard_normal((B, H, W, Cc)).astype(np.float32)
    want_t = torch.tensor(tex, dtype=torch.float64, requires_grad=True)
    want_uv = torch.tensor(uv, dtype=torch.float64, requires_grad=True)
    want = _grid_sample(want_t, want_uv)
    (want * torch.tensor(G, dtype=torch.float64)).sum().backward()
    got = tc.sample_restated(tex, uv, None, "clamp", np.float64)
    dtex, duv, kink = tc.sample_grads_restated(tex, uv, G, None, "clamp", np.float64)
    print(f"\nvalue {np.abs(got - want.detach().numpy()).max():.2e} dtex {np.abs(dtex - want_t.grad.numpy()).max():.2e} "
          f"duv {np.abs(duv - want_uv.grad.numpy())[~kink].max():.2e} kinks {int(kink.sum())}")
    assert np.abs(got - want.detach().numpy()).max() <= 1e-12
    assert np.abs(dtex - want_t.grad.numpy()).max() <= 1e-12 * max(1, H * W)
    assert np.abs(duv - want_uv.grad.numpy())[~kink].max() <= 1e-12 * max(Ht, Wt) and kink.sum() <= max(2, 0.01 * kink.size)


def test_wrap_restatement_equals_clamp_on_a_tiled_texture():
    rng = np.random.default_rng(6)
    for (Ht, Wt), Cc in (((5, 3), 3), ((1, 4), 1), ((2, 2), 8)):
        tex = rng.standard_normal((2, Ht, Wt, Cc)).astype(np.float32)
        size = np.array([Wt, Ht])                                               # the footprint must stay inside the 3 x 3 tiling
        uv = rng.uniform(-1 + 0.5 / size + 0.01, 2 - 1.5 / size - 0.01, (2, 9, 11, 2))
        G = rng.standard_normal((2, 9, 11, Cc)).astype(np.float32)
        tiled = np.tile(tex, (1, 3, 3, 1))
        got = tc.sample_restated(tex, uv, None, "wrap", np.float64)
        want = tc.sample_restated(tiled, (uv + 1) / 3, None, "clamp", np.float64)
        assert np.abs(got - want).max() <= 1e-12
        dtex, duv, kink = tc.sample_grads_restated(tex, uv, G, None, "wrap", np.float64)
        dt_tiled, duv_tiled, kink2 = tc.sample_grads_restated(tiled, (uv + 1) / 3, G, None, "clamp", np.float64)
        folded = dt_tiled.reshape(2, 3, Ht, 3, Wt, Cc).sum((1, 3))
        assert np.abs(dtex - folded).max() <= 1e-12 and np.abs(duv - duv_tiled / 3)[~(kink | kink2)].max() <= 1e-11
    # negative indices wrap, the fp32 path included: u = -0.5 / Wt is texel -1 = Wt - 1
    tex = np.arange(4, dtype=np.float32).reshape(1, 1, 4, 1)
    uv = np.array([[-0.5 / 4, 0.5], [4.5 / 4, 0.5], [-100.0 + 2.5 / 4, 0.5]], np.float32).reshape(1, 1, 3, 2)
    assert tc.sample_restated(tex, uv, None, "wrap", np.float32).reshape(-1).tolist() == [3.0, 0.0, 2.0]
    assert tc.sample_restated(tex, uv, None, "clamp", np.float32).reshape(-1).tolist() == [0.0, 3.0, 0.0]


def test_fp32_restatement_skips_and_orients_as_the_contract_says():
    tex = np.arange(6, dtype=np.float32).reshape(1, 2, 3, 1)                     # row 0 = (0, 1, 2) is v = 0
    centres = np.array([[[(j + 0.5) / 3, (i + 0.5) / 2] for j in range(3)] for i in range(2)], np.float32)[None]
    assert np.array_equal(tc.sample_restated(tex, centres)[0, ..., 0], tex[0, ..., 0])
    uv = np.array([[np.nan, 0.5], [0.5, np.inf], [3e38, 0.5], [0.5, 0.5]], np.float32).reshape(1, 1, 4, 2)
    rast = np.ones((1, 1, 4, 4), np.float32)
    rast[0, 0, 3, 3] = 0
    out = tc.sample_restated(tex, uv, rast)
    assert not out.any() and not np.isnan(out).any()
    dtex, duv, _ = tc.sample_grads_restated(tex, uv, np.ones((1, 1, 4, 1), np.float32), rast)
    assert not dtex.any() and not duv.any()


@pytest.mark.parametrize("resolution", [16, 64, 1024])
@pytest.mark.parametrize("n_faces", [1, 2, 3, 7, 1000])
def test_face_atlas_keeps_every_bilinear_footprint_inside_its_tile(n_faces, resolution):
    from meshdiffusion_amd import texture
    n, s = texture.atlas_layout(n_faces, resolution)
    assert n * n >= (n_faces + 1) // 2 > (n - 1) * (n - 1) - (n == 1) and s == resolution // n
    if s < 4:                                                                   # 2 gutter + 2 with the default gutter
        with pytest.raises(ValueError, match="raise the resolution"):
            texture.face_atlas(n_faces, resolution)
        return
    uvs, uv_idx = texture.face_atlas(n_faces, resolution)
    assert uvs.dtype == torch.float32 and tuple(uvs.shape) == (4 * ((n_faces + 1) // 2), 2)
    assert uv_idx.dtype == torch.int64 and tuple(uv_idx.shape) == (n_faces, 3)
    quad = torch.tensor([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])         # any geometry: only the atlas is looked at
    verts = quad.repeat((n_faces + 1) // 2, 1)
    bake = tc.render_uv_cpu(verts, uv_idx, uvs, uv_idx, resolution)              # faces = uv_idx: pos is the quad's corner mix
    face, cov = bake["face_id"], bake["mask"] > 0.5
    assert set(np.unique(face[cov]).tolist()) == set(range(n_faces))             # every face owns a texel
    uv = bake["uv"][cov].astype(np.float32).reshape(1, 1, -1, 2)                 # the uv a render interpolates at the texel
    live, ix0, ix1, iy0, iy1, *_ = tc.tap(uv, None, resolution, resolution, "clamp", np.float32)
    tile = face[cov] // 2
    col, row = tile % n, tile // n
    assert live.all()
    for ix, iy in ((ix0, iy0), (ix1, iy0), (ix0, iy1), (ix1, iy1)):
        assert np.array_equal(ix.reshape(-1) // s, col) and np.array_equal(iy.reshape(-1) // s, row)
    # a covered texel keeps `gutter` texels to the border of its tile
    ii, jj = np.nonzero(cov)
    assert (jj % s >= 1).all() and (jj % s <= s - 2).all() and (ii % s >= 1).all() and (ii % s <= s - 2).all()
    for gutter in (0, 2):
        if s >= 2 * gutter + 2:
            u2, _ = texture.face_atlas(n_faces, resolution, gutter)
            local = (u2.double() * resolution) % s
            assert float(local.min()) >= gutter - 1e-3 or gutter == 0
    with pytest.raises(ValueError):
        texture.face_atlas(0, resolution)


def test_new_exports_refuse_bad_arguments_without_a_gpu(hip_lib):
    from meshdiffusion_amd import _lib, build
    assert "texture.hip" in build.SOURCES and _lib.ABI_VERSION == 16
    src = open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "texture.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "THE TEXTURE CONTRACT" in src and "atomicAdd" not in src and "__shared__" not in src
    nul, one, odd16, odd8, odd4 = C.c_void_p(0), C.c_void_p(64), C.c_void_p(72), C.c_void_p(68), C.c_void_p(66)

    def check(fn, ok, pointers=(), sizes=(), unsupported=(), misaligned=(), bad=()):
        for k in pointers:
            a = list(ok); a[k] = nul
            assert fn(*a) == -1, (fn.__name__, "null", k)
        for k in sizes:
            for v in (0, -3):
                a = list(ok); a[k] = v
                assert fn(*a) == -1, (fn.__name__, "size", k, v)
        for k, v in unsupported:
            a = list(ok); a[k] = v
            assert fn(*a) == -2, (fn.__name__, "unsupported", k, v)
        for k, p in misaligned:
            a = list(ok); a[k] = p
            assert fn(*a) == -1, (fn.__name__, "misaligned", k)
        for k, v in bad:
            a = list(ok); a[k] = v
            assert fn(*a) == -1, (fn.__name__, "bad", k, v)

    # md_texture_sample(tex, uv, rast, T, Ht, Wt, C, B, H, W, boundary, out, stream)
    ok = [one, one, one, 1, 32, 48, 3, 2, 16, 24, 0, one, nul]
    check(hip_lib.md_texture_sample, ok, pointers=(0, 1, 11), sizes=(3, 4, 5, 7, 8, 9),
          unsupported=((6, 0), (6, 9), (6, -1), (4, 2049), (5, 2049), (7, 65), (8, 2049), (9, 2049)),
          misaligned=((0, odd16), (11, odd16), (2, odd16), (1, odd8)), bad=((3, 3), (10, 2), (10, -1)))
    # md_texture_codes(uv, rast, T, Ht, Wt, B, H, W, boundary, dest, stream)
    ok = [one, one, 1, 32, 48, 2, 16, 24, 1, one, nul]
    check(hip_lib.md_texture_codes, ok, pointers=(0, 9), sizes=(2, 3, 4, 5, 6, 7),
          unsupported=((3, 2049), (4, 2049), (5, 65), (6, 2049), (7, 2049)), misaligned=((0, odd8), (1, odd16), (9, odd16)),
          bad=((2, 3), (8, 2)))
    # md_texture_sample_bwd(tex, uv, rast, grad_out, ptr, order, T, Ht, Wt, C, B, H, W, boundary, dtex, duv, stream)
    ok = [one, one, one, one, one, one, 1, 32, 48, 3, 2, 16, 24, 0, one, one, nul]
    check(hip_lib.md_texture_sample_bwd, ok, pointers=(0, 1, 3, 4, 5), sizes=(6, 7, 8, 10, 11, 12),
          unsupported=((9, 0), (9, 9), (7, 2049), (8, 2049), (10, 65), (11, 2049), (12, 2049)),
          misaligned=((0, odd16), (3, odd16), (2, odd16), (14, odd16), (1, odd8), (15, odd8), (4, odd4), (5, odd4)), bad=((6, 3), (13, 2)))
    a = list(ok); a[14] = a[15] = nul
    assert hip_lib.md_texture_sample_bwd(*a) == -1                             # nothing to compute
    # md_texture_dilate(tex, mask, Ht, Wt, C, out_tex, out_mask, stream)
    far = [C.c_void_p(1 << 30), C.c_void_p(2 << 30), C.c_void_p(3 << 30), C.c_void_p(4 << 30)]
    ok = [far[0], far[1], 32, 48, 3, far[2], far[3], nul]
    check(hip_lib.md_texture_dilate, ok, pointers=(0, 1, 5, 6), sizes=(2, 3), unsupported=((4, 0), (4, 9), (2, 2049), (3, 2049)),
          misaligned=((0, C.c_void_p((1 << 30) + 8)), (5, C.c_void_p((3 << 30) + 8)), (1, C.c_void_p((2 << 30) + 2))),
          bad=((5, far[0]), (6, far[1]), (5, C.c_void_p((1 << 30) + 32 * 48 * 12 - 16)), (6, far[0]), (5, far[1])))
    # md_texture_project(pos, nrm, texmask, image, depth, viewmask, mvp, campos, Ht, Wt, V, H, W, bias, cos_min, power, color, weight, stream)
    ok = [one] * 8 + [32, 48, 4, 16, 24, C.c_float(0.01), C.c_float(0.1), C.c_float(2.0), one, one, nul]
    check(hip_lib.md_texture_project, ok, pointers=(0, 1, 2, 3, 4, 5, 6, 7, 16, 17), sizes=(8, 9, 10, 11, 12),
          unsupported=((10, 65), (8, 2049), (9, 2049), (11, 2049), (12, 2049)), misaligned=((0, odd4), (17, odd4)),
          bad=((13, C.c_float(float("nan"))), (15, C.c_float(float("nan")))))


def test_host_functions_check_their_arguments(monkeypatch):
    from meshdiffusion_amd import _lib, texture
    tex, uv = torch.zeros(4, 4, 3), torch.zeros(1, 8, 8, 2)
    with pytest.raises(_lib.MeshDiffusionHipError):
        texture.sample(tex, uv)                                                 # CPU tensors: no fallback
    with pytest.raises(_lib.MeshDiffusionHipError):
        texture.dilate(tex, torch.zeros(4, 4), 1)
    with pytest.raises(_lib.MeshDiffusionHipError):
        texture.render_uv(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]), torch.zeros(4, 2), torch.tensor([[0, 1, 2]]), 8)
    monkeypatch.setattr(texture, "_gpu_only", lambda t, what: None)
    for bad_tex in (torch.zeros(3, 4, 4, 3), torch.zeros(4, 3), torch.zeros(0, 4, 3)):
        with pytest.raises(ValueError):
            texture.sample(bad_tex, uv)
    with pytest.raises(ValueError):
        texture.sample(tex, torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError):
        texture.sample(tex, uv, rast=torch.zeros(1, 8, 7, 4))
    with pytest.raises(ValueError):
        texture.sample(tex, uv, boundary="mirror")
    for shape in ((4, 4, 9), (4, 4, 0), (2049, 4, 3)):
        with pytest.raises(_lib.MeshDiffusionHipError):
            texture.sample(torch.zeros(shape), uv)
    with pytest.raises(_lib.MeshDiffusionHipError):
        texture.sample(tex, torch.zeros(65, 2, 2, 2))


def test_textured_obj_round_trip(tmp_path):
    from meshdiffusion_amd import mesh_export, texture
    verts, faces = tc.cube_mesh(2)
    uvs, uv_idx = texture.face_atlas(faces.shape[0], 64)
    tex = torch.tensor(tc.smooth_color(np.random.default_rng(3).uniform(-1, 1, (64, 64, 3))), dtype=torch.float32)
    obj, mtl, png = texture.save_textured_obj(str(tmp_path / "mesh.obj"), verts, faces, uvs, uv_idx, tex)
    mesh_export.save_obj(str(tmp_path / "plain.obj"), verts, faces)
    lines, plain = open(obj).read().split("\n"), open(tmp_path / "plain.obj").read().split("\n")
    assert [l for l in lines if l.startswith("v ")] == [l for l in plain if l.startswith("v ")]
    f_lines = [l for l in lines if l.startswith("f ")]
    assert [" ".join(c.split("/")[0] for c in l.split()[1:]) for l in f_lines] == [l[2:] for l in plain if l.startswith("f ")]
    vt = np.array([[float(c) for c in l.split()[1:]] for l in lines if l.startswith("vt ")])
    assert vt.shape == (uvs.shape[0], 2)
    assert np.abs(vt[:, 0] - uvs[:, 0].numpy()).max() < 1e-6 and np.abs(vt[:, 1] - (1 - uvs[:, 1].numpy())).max() < 1e-6   # v flipped
    idx = np.array([[int(c.split("/")[1]) - 1 for c in l.split()[1:]] for l in f_lines])
    assert np.array_equal(idx, uv_idx.numpy())
    assert lines[0] == "mtllib mesh.mtl" and "usemtl material_0" in lines
    assert "map_Kd mesh_kd.png" in open(mtl).read() and "newmtl material_0" in open(mtl).read()
    img = mesh_export.load_png(png)
    assert np.array_equal(img, np.clip(np.rint(tex.numpy().astype(np.float64) * 255), 0, 255).astype(np.uint8))   # row 0 on top, unflipped
    v2, f2 = mesh_export.load_obj(obj)
    assert np.array_equal(f2, faces.numpy()) and np.abs(v2 - verts.numpy()).max() < 1e-6


def test_fixture_is_small_and_holds_every_bar():
    path = os.path.join(GOLD, "texture.npz")
    assert os.path.getsize(path) < 64 * 1024
    gold = np.load(path)
    assert all(gold[k].size <= 8 for k in gold.files)                           # scalars, no images
    for case in tc.BWD_CASES:
        for q in ("dtex", "duv"):
            assert 0 <= float(gold[f"bwd/{tc.sample_case_id(case)}/ref_err_{q}"]) < 1e-5, (case, q)
    for name in tc.dilate_cases():
        assert 0 <= float(gold[f"dilate/{name}/ref_err"]) < 1e-6
    for case in tc.PROJECT_CASES:
        cid = tc.project_case_id(case)
        assert 0 <= float(gold[f"project/{cid}/left_out"]) <= tc.MAX_LEFT_OUT and 0 < float(gold[f"project/{cid}/ref_err_color"]) < 1e-5
    assert 0 < float(gold["round_trip/cpu_mean_err"]) < 0.01 < float(gold["round_trip/cpu_err"]) < 0.5 and float(gold["round_trip/seen"]) > 0.9
