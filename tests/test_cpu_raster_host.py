"""Host side of the depth rasteriser (meshdiffusion_amd/render.py, csrc/raster.hip) without a GPU: the camera helpers against
the reference's matrices in tests/golden/raster.npz, the tie rule of the restatement, depth_loss against a literal restatement,
the silhouette carve on a CPU stub, argument checking, and the export tables."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import raster_cases as rc
from conftest import GOLD


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "raster.npz"))


def test_new_exports_are_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import build, render
    assert "raster.hip" in build.SOURCES
    for name in ("perspective", "translate", "rotate_x", "rotate_y", "random_rotation_translation", "xfm_points", "rasterize",
                 "render_depth", "depth_loss", "make_targets", "carve_outside_silhouette", "fit_to_views"):
        assert callable(getattr(render, name)), name


def test_new_exports_refuse_bad_arguments_without_a_gpu(hip_lib):
    nul, one, odd = C.c_void_p(0), C.c_void_p(64), C.c_void_p(68)

    def refuses(fn, ok, pointers, sizes):
        for k in pointers:
            a = list(ok); a[k] = nul
            assert fn(*a) == -1, (fn.__name__, k)
        for k in sizes:
            for bad in (0, -3):
                a = list(ok); a[k] = bad
                assert fn(*a) == -1, (fn.__name__, k, bad)

    def unsupported(fn, ok, b, f, h, w):
        for k, v in ((b, 65), (f, 1 << 24), (h, 2049), (w, 2049)):
            a = list(ok); a[k] = v
            assert fn(*a) == -2, (fn.__name__, k)

    # md_raster_bin_count(pos_clip, faces, B, V, F, H, W, counts, stream)
    ok = [one, one, 2, 100, 300, 64, 48, one, nul]
    refuses(hip_lib.md_raster_bin_count, ok, (0, 1, 7), (2, 3, 4, 5, 6))
    unsupported(hip_lib.md_raster_bin_count, ok, 2, 4, 5, 6)
    a = list(ok); a[0] = odd
    assert hip_lib.md_raster_bin_count(*a) == -1                      # float4 loads
    # md_raster_bin_emit(pos_clip, faces, offsets, B, V, F, H, W, total, pair_tile, pair_face, stream)
    ok = [one, one, one, 2, 100, 300, 64, 48, 1000, one, one, nul]
    refuses(hip_lib.md_raster_bin_emit, ok, (0, 1, 2, 9, 10), (3, 4, 5, 6, 7, 8))
    unsupported(hip_lib.md_raster_bin_emit, ok, 3, 5, 6, 7)
    a = list(ok); a[8] = 1 << 31
    assert hip_lib.md_raster_bin_emit(*a) == -2                       # more than 2^31 - 1 pairs
    # md_raster_tiles(pos_clip, faces, tile_ptr, tile_faces, B, V, F, H, W, rast1, rast2, stream)
    ok = [one, one, one, one, 2, 100, 300, 64, 48, one, one, nul]
    refuses(hip_lib.md_raster_tiles, ok, (0, 1, 2, 3, 9, 10), (4, 5, 6, 7, 8))
    unsupported(hip_lib.md_raster_tiles, ok, 4, 6, 7, 8)
    a = list(ok); a[10] = odd
    assert hip_lib.md_raster_tiles(*a) == -1                          # 16-byte stores
    # md_raster_depth(rast1, rast2, verts, faces, campos, B, V, F, H, W, depth1, depth2, mask1, mask2, stream)
    ok = [one] * 5 + [2, 100, 300, 64, 48, one, one, one, one, nul]
    refuses(hip_lib.md_raster_depth, ok, (0, 1, 2, 3, 4, 10, 11, 12, 13), (5, 6, 7, 8, 9))
    unsupported(hip_lib.md_raster_depth, ok, 5, 7, 8, 9)
    # md_raster_depth_bwd(cov, n_cov, rast1, rast2, gd1, gd2, pos_clip, verts, faces, mvp, campos, ptr, order, B, V, F, H, W,
    #                     corner_grad, dverts, stream)
    ok = [one, 500] + [one] * 11 + [2, 100, 300, 64, 48, one, one, nul]
    refuses(hip_lib.md_raster_depth_bwd, ok, (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 18, 19), (13, 14, 15, 16, 17))
    unsupported(hip_lib.md_raster_depth_bwd, ok, 13, 15, 16, 17)
    a = list(ok); a[1] = -1
    assert hip_lib.md_raster_depth_bwd(*a) == -1
    a = list(ok); a[1] = 800_000_000
    assert hip_lib.md_raster_depth_bwd(*a) == -2                      # 3 n_cov must fit the int32 corner codes


def test_camera_helpers_return_the_reference_matrices(gold):
    from meshdiffusion_amd import render
    for helper in ("perspective", "translate", "rotate_x", "rotate_y"):
        args, want = gold[f"cam/{helper}/args"], gold[f"cam/{helper}/out"]
        assert len(args) >= 2
        for a, w in zip(args, want):
            got = getattr(render, helper)(*[float(x) for x in a])
            assert got.dtype == torch.float32 and got.shape == (4, 4)
            assert np.array_equal(got.numpy(), w), (helper, a)
    np.random.seed(int(gold["cam/rrt/seed"]))
    for w in gold["cam/rrt/out"]:
        assert np.array_equal(render.random_rotation_translation(float(gold["cam/rrt/t"])).numpy(), w)
    # the camera of the cases is the product of the helpers, left to right
    for a, (H, W) in ((0.7, (64, 64)), (2.1, (40, 72))):
        mvp = render.perspective(np.deg2rad(45.0), W / H, 0.1, 1000.0) @ render.translate(0, 0, -3.0) @ render.rotate_x(-0.4) @ render.rotate_y(a)
        m, campos = rc.camera(a, H, W)
        assert torch.equal(mvp, m)
        assert abs(float(campos.norm()) - 3.0) < 1e-5


def test_xfm_points_is_the_matrix_product_and_differentiable():
    from meshdiffusion_amd import render
    g = torch.Generator().manual_seed(1)
    p = torch.randn(7, 3, generator=g, dtype=torch.float64, requires_grad=True)
    m = torch.randn(3, 4, 4, generator=g, dtype=torch.float64)
    out = render.xfm_points(p[None], m)
    want = torch.matmul(torch.nn.functional.pad(p[None], (0, 1), value=1.0), m.transpose(1, 2))
    assert out.shape == (3, 7, 4) and torch.allclose(out, want, atol=1e-13)
    assert torch.equal(render.xfm_points(p.detach().float(), m.float()), rc.xfm_points_restated(p.detach().float(), m.float()))
    out.sum().backward()
    assert torch.allclose(p.grad, m[:, :, :3].sum((0, 1)).expand(7, 3), atol=1e-12)
    with pytest.raises(ValueError):
        render.xfm_points(torch.zeros(2, 5, 3), m)


def test_tie_rule_gives_every_pixel_of_a_fan_exactly_one_owner():
    """8 triangles of mixed orientation around a pixel centre, every spoke through pixel centres: one owner per pixel."""
    pc, faces, H, W = rc.small_case("fan")
    X, Y, ok = rc.snap(pc, H, W)
    assert bool(ok.all()) and int(X[0, 0]) == 256 * 4 + 128 and int(Y[0, 0]) == 256 * 4 + 128
    owners = torch.zeros(H, W, dtype=torch.int64)
    for f in range(faces.shape[0]):
        r = rc.rasterize_restated(pc, faces[f:f + 1], H, W)
        owners += (r["ids"][0, 0] > 0).long()
    r = rc.rasterize_restated(pc, faces, H, W)
    assert r["on_edge"] >= 8 + 2 * 8                          # the hub pixel on all 8 triangles, and centres along the spokes
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[1:8, 1:8] = True                                   # |offset| <= 900 / 256 pixels around pixel (4, 4): columns 1..7
    assert bool((owners[inside] == 1).all()) and bool((owners[~inside] == 0).all())
    assert bool((r["ids"][0, 1] == 0).all()) and bool(((r["ids"][0, 0] > 0) == inside).all())
    # the quad: the shared diagonal and the outer edges pass through centres; top / left edges own them, bottom / right do not
    pc, faces, H, W = rc.small_case("quad")
    r = rc.rasterize_restated(pc, faces, H, W)
    got = r["ids"][0, 0] > 0
    want = torch.zeros(H, W, dtype=torch.bool)
    want[1:6, 1:6] = True
    assert r["on_edge"] > 0 and bool((r["ids"][0, 1] == 0).all())
    assert bool((got == want).all())


def test_restatement_small_cases():
    pc, faces, H, W = rc.small_case("huge")
    X, Y, _ = rc.snap(pc, H, W)
    assert int(X.abs().max()) == 2 ** 22 and int(Y.abs().max()) == 2 ** 22
    assert bool((rc.rasterize_restated(pc, faces, H, W)["ids"][0, 0] == 1).all())
    pc, faces, H, W = rc.small_case("skipped")
    ids = rc.rasterize_restated(pc, faces, H, W)["ids"]
    assert set(ids.unique().tolist()) == {0, 3}
    pc, faces, H, W = rc.small_case("empty")
    assert not bool(rc.rasterize_restated(pc, faces, H, W)["ids"].any())
    pc, faces, H, W = rc.small_case("coincident")
    ids = rc.rasterize_restated(pc, faces, H, W)["ids"]
    cov = ids[0, 0] > 0
    assert int(cov.sum()) > 10 and bool((ids[0, 0][cov] == 1).all()) and bool((ids[0, 1][cov] == 2).all())


def test_depth_loss_against_the_literal_restatement():
    from meshdiffusion_amd import render
    g = torch.Generator().manual_seed(3)
    shape = (3, 9, 11, 1)
    t_depth = 2.5 + torch.rand(shape, generator=g)
    t_second = t_depth + torch.rand(shape, generator=g) * 0.01          # some closer than 5e-3: the proximity mask
    t_second[0, :3] = -1.0                                              # no second layer: the valid mask
    mask = (torch.rand(shape, generator=g) > 0.3).float()
    mask[1, 4:6] = 0.5                                                  # an antialiased target mask counts as 0
    depth = t_depth + torch.randn(shape, generator=g) * 0.3
    depth[2, :2] = 20.0                                                 # uncovered prediction: the d >= 1 branch
    second = t_second + torch.randn(shape, generator=g) * 0.3
    second[2, 5:] = -1.0
    second[1, :1] = t_second[1, :1] + 15.0                              # 0.1 * 15 >= 1: the branch in the second term
    target = {"depth": t_depth, "depth_second": t_second, "mask_cont": mask}
    vals = {}
    for it in (0, 9999, 10000, 20000):
        d = depth.clone().requires_grad_(True)
        got = render.depth_loss({"depth": d, "depth_second": second}, target, it)
        want = rc.depth_loss_restated(depth.double(), second.double(), t_depth.double(), t_second.double(), mask.double(), it)
        assert got.dtype == torch.float32 and abs(float(got.detach()) - float(want)) <= 2e-6 * float(want), it
        got.backward()
        assert bool(torch.isfinite(d.grad).all()) and float(d.grad.abs().sum()) > 0
        vals[it] = float(got.detach())
    assert abs(vals[9999] / vals[10000] - 100.0) < 1e-3 and vals[0] == vals[9999] and vals[10000] == vals[20000]
    big = ((depth - t_depth).abs() * (mask[..., 0:1] == 1).float() * (t_second >= 0).float()) >= 1
    assert int(big.sum()) > 0


class _StubGeometry:
    """The members carve_outside_silhouette touches, on the CPU."""

    def __init__(self, verts):
        self.verts = verts
        self.sdf = torch.nn.Parameter(torch.full((verts.shape[0],), -0.5))
        self.deform = torch.nn.Parameter(torch.full_like(verts, 0.1))

    def get_deformed(self):
        return self.verts + 0.01 * self.deform


def test_carve_outside_silhouette_on_a_cpu_stub():
    from meshdiffusion_amd import render
    H = W = 64
    mvp, campos = rc.cameras((0.0, math.pi / 2), H, W)
    lin = torch.linspace(-1.0, 1.0, 9)
    verts = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3)
    geo = _StubGeometry(verts)
    # the silhouette of a ball of radius 0.4 in both views
    mask = torch.zeros(2, H, W, 1)
    clip = render.xfm_points(geo.get_deformed().detach()[None], mvp)
    rad_px = 0.4 / (3.0 * np.tan(np.deg2rad(22.5))) * (W / 2)
    jj, ii = torch.meshgrid(torch.arange(W), torch.arange(H), indexing="xy")
    mask[:, :, :, 0] = (((jj - (W - 1) / 2) ** 2 + (ii - (H - 1) / 2) ** 2) <= rad_px ** 2).float()
    target = {"mask_cont": mask, "mvp": mvp, "campos": campos, "resolution": [H, W]}
    n = render.carve_outside_silhouette(geo, target)
    # restated: a vertex is carved when, in some view, the 11 x 11 window around its pixel holds no mask pixel
    ndc = clip[..., :2] / clip[..., 3:4]
    px = torch.round((ndc[..., 0] * 0.5 + 0.5).clip(0, 1) * (W - 1)).long()
    py = torch.round((ndc[..., 1] * 0.5 + 0.5).clip(0, 1) * (H - 1)).long()
    want = torch.zeros(verts.shape[0], dtype=torch.bool)
    for k in range(2):
        for v in range(verts.shape[0]):
            win = mask[k, max(py[k, v] - 5, 0):py[k, v] + 6, max(px[k, v] - 5, 0):px[k, v] + 6, 0]
            want[v] |= not bool(win.any())
    assert 0 < n == int(want.sum()) < verts.shape[0]
    assert bool((geo.sdf.data[want] == 1e-2).all()) and bool((geo.deform.data[want] == 0).all())
    assert bool((geo.sdf.data[~want] == -0.5).all()) and bool((geo.deform.data[~want] == 0.1).all())
    assert bool(want[verts.norm(dim=1) > 1.5].all()) and not bool(want[verts.norm(dim=1) < 0.3].any())


def test_host_functions_check_their_arguments():
    from meshdiffusion_amd import _lib, render
    pc = torch.zeros(1, 4, 4)
    f = torch.tensor([[0, 1, 2]])
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.rasterize(pc, f, 8)                                      # CPU tensor: no fallback
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.render_depth(torch.zeros(4, 3), f, torch.eye(4)[None], torch.zeros(1, 3), 8)
    with pytest.raises(_lib.MeshDiffusionHipError):
        render._resolution((4096, 8))
    with pytest.raises(ValueError):
        render._resolution((0, 8))
    assert render._resolution(8) == (8, 8) and render._resolution([40, 72]) == (40, 72)
    with pytest.raises(ValueError):
        render._check_faces(torch.tensor([[0, 1, 4]]), 4)
    with pytest.raises(ValueError):
        render._check_faces(torch.tensor([[0, 1]]), 4)
    assert render._check_faces(torch.zeros(0, 3, dtype=torch.int64), 4).shape == (0, 3)
    with pytest.raises(ValueError):
        render._check_clip(torch.zeros(1, 4, 3))
    with pytest.raises(_lib.MeshDiffusionHipError):
        render._check_clip(torch.zeros(65, 4, 4))


def test_fixture_is_small_and_its_fit_falls(gold):
    assert os.path.getsize(os.path.join(GOLD, "raster.npz")) < 64 * 1024
    l32, l64 = gold["fit/loss32"], gold["fit/loss64"]
    assert tuple(gold["fit/steps"]) == rc.FIT_STEPS and l64[-1] < 0.5 * l64[0] and l32[-1] < 0.5 * l32[0]
    for case in rc.MESH_CASES:
        cid = rc.case_id(case)
        for k in ("uv", "zf", "depth"):
            assert 0 < float(gold[f"case/{cid}/ref_err_{k}"]) < 1e-4, (cid, k)
        assert (f"case/{cid}/ref_err_dverts" in gold.files) == (case in rc.GRAD_CASES)


@pytest.mark.parametrize("case", [c for c in rc.MESH_CASES if c[0] != "noise"], ids=rc.case_id)
def test_input_conditions_left_out_pixels_stay_under_the_cap(case, gold):
    """The exclusions the GPU tests may make are rare on the cases (the noise case is checked on the GPU, where it is rendered)."""
    name, H, W = case
    verts, faces = rc.mesh(name)
    mvp, _ = rc.cameras(rc.ANGLES, H, W)
    r = rc.rasterize_restated(rc.xfm_points_restated(verts, mvp), faces, H, W)
    _, _, covered = rc.check_caps(r, rc.case_id(case))
    assert [int(covered[:, 0].sum()), int(covered[:, 1].sum())] == gold[f"case/{rc.case_id(case)}/covered"].tolist()
