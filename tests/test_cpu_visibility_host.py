"""Host side of the visible-tet labelling and the single-view fit (csrc/visibility.hip, meshdiffusion_amd/singleview.py) without a
GPU: the restatements of tests/visibility_cases.py against brute force on a hand-made layer, the export tables, argument
refusal, the plain-torch carve, the fixture, and the way of a `single_view_partial` dict through `evaler.cond_gen`'s scatter."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import raster_cases as rc
import visibility_cases as vc
from conftest import GOLD, ROOT


def test_new_exports_are_declared_everywhere(hip_lib):
    from meshdiffusion_amd import build, dmtet, singleview
    header = open(os.path.join(ROOT, "include", "meshdiffusion_hip.h")).read()
    assert "visibility.hip" in build.SOURCES and "THE VISIBILITY CONTRACT" in header
    src = open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "visibility.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "THE VISIBILITY CONTRACT" in src and "atomic" not in src.replace("no atomics", "")
    assert "__fdiv_rn" in src and "rintf" in src and "Deviation" in src
    for name in ("window_min_depth", "visible_tets", "label_vertices", "single_view_partial", "init_with_gt_surface",
                 "carve_single_view", "fit_single_view"):
        assert callable(getattr(singleview, name)), name
    assert callable(dmtet.DMTetGeometry.init_with_gt_surface)
    assert singleview.MAX_RADIUS == 15 and singleview.EMPTY_DEPTH == vc.EMPTY


def test_new_exports_refuse_bad_arguments_without_a_gpu(hip_lib):
    nul, one, odd = C.c_void_p(0), C.c_void_p(64), C.c_void_p(68)
    # md_window_min(rast, B, H, W, radius, dmin, stream)
    ok = [one, 2, 40, 72, 7, one, nul]
    for k, bad, want in ((0, nul, -1), (5, nul, -1), (0, odd, -1), (1, 0, -1), (2, -1, -1), (3, 0, -1), (4, -1, -1), (4, 16, -2),
                         (1, 65, -2), (2, 2049, -2), (3, 2049, -2)):
        a = list(ok); a[k] = bad
        assert hip_lib.md_window_min(*a) == want, ("md_window_min", k, bad)
    # md_tet_visibility(dmin, centres, mvp, B, T, H, W, visible, stream)
    ok = [one, one, one, 2, 1000, 40, 72, one, nul]
    for k, bad, want in ((0, nul, -1), (1, nul, -1), (2, nul, -1), (7, nul, -1), (3, 0, -1), (4, 0, -1), (5, 0, -1), (6, -2, -1),
                         (3, 65, -2), (4, 1 << 31, -2), (5, 4096, -2)):
        a = list(ok); a[k] = bad
        assert hip_lib.md_tet_visibility(*a) == want, ("md_tet_visibility", k, bad)
    # md_rast_mark_tets(rast, face_tet, B, H, W, F, T, rast_tet, stream)
    ok = [one, one, 2, 40, 72, 300, 1000, one, nul]
    for k, bad, want in ((0, nul, -1), (1, nul, -1), (7, nul, -1), (1, odd, -1), (5, 0, -1), (6, 0, -1), (5, 1 << 24, -2),
                         (6, 1 << 31, -2), (2, 65, -2)):
        a = list(ok); a[k] = bad
        assert hip_lib.md_rast_mark_tets(*a) == want, ("md_rast_mark_tets", k, bad)
    # md_tets_mark_verts(visible, rast_tet, indices, B, T, N, vis, vis_rast, stream); rast_tet may be null
    ok = [one, nul, one, 2, 1000, 500, one, one, nul]
    for k, bad, want in ((0, nul, -1), (2, nul, -1), (6, nul, -1), (7, nul, -1), (2, odd, -1), (3, 0, -1), (4, 0, -1), (5, -4, -1),
                         (3, 65, -2), (4, 1 << 31, -2), (5, 1 << 31, -2)):
        a = list(ok); a[k] = bad
        assert hip_lib.md_tets_mark_verts(*a) == want, ("md_tets_mark_verts", k, bad)


def test_python_entry_points_refuse_cpu_tensors_bad_radii_and_bad_shapes(monkeypatch):
    from meshdiffusion_amd import _lib, singleview as sv
    rast = vc.hand_rast()
    centres, mvp = torch.zeros(5, 3), torch.eye(4)[None]
    tets = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]])
    for call in (lambda: sv.window_min_depth(rast), lambda: sv.visible_tets(rast, centres, mvp),
                 lambda: sv.label_vertices(torch.zeros(1, 2, dtype=torch.bool), rast, torch.zeros(3, dtype=torch.long), tets, 5),
                 lambda: sv.window_min_depth(rast, radius=16), lambda: sv.visible_tets(rast, centres, mvp, radius=16)):
        with pytest.raises(_lib.MeshDiffusionHipError):
            call()                                                            # CPU tensors: no fallback; 16: MD_ERR_UNSUPPORTED
    geo = types.SimpleNamespace(sdf=torch.zeros(5), deform=torch.zeros(5, 3))
    with pytest.raises(_lib.MeshDiffusionHipError):
        sv.single_view_partial(geo, {})
    with pytest.raises(_lib.MeshDiffusionHipError):
        sv.init_with_gt_surface(geo, torch.zeros(3, 3), torch.tensor([[0, 1, 2]]), torch.zeros(3))
    with pytest.raises(_lib.MeshDiffusionHipError):
        sv.fit_single_view(geo, {}, 1)
    monkeypatch.setattr(sv, "_gpu_only", lambda t, what: None)                 # the shape checks come before any launch
    monkeypatch.setattr("meshdiffusion_amd.fit._gpu_only", lambda t, what: None)    # where fit_single_view lives
    for call in (lambda: sv.window_min_depth(rast[0]), lambda: sv.window_min_depth(rast[..., :3]), lambda: sv.window_min_depth(rast, -1),
                 lambda: sv.window_min_depth(rast, 2.5), lambda: sv.visible_tets(rast, torch.zeros(5), mvp),
                 lambda: sv.visible_tets(rast, torch.zeros(0, 3), mvp), lambda: sv.visible_tets(rast, centres, torch.eye(4)),
                 lambda: sv.visible_tets(rast, centres, torch.eye(4)[None].expand(2, 4, 4)),
                 lambda: sv.label_vertices(torch.zeros(2, 2, dtype=torch.bool), rast, torch.zeros(3, dtype=torch.long), tets, 5),
                 lambda: sv.label_vertices(torch.zeros(1, 3, dtype=torch.bool), rast, torch.zeros(3, dtype=torch.long), tets, 5),
                 lambda: sv.label_vertices(torch.zeros(1, 2, dtype=torch.bool), rast, torch.tensor([0, 2]), tets, 5),
                 lambda: sv.label_vertices(torch.zeros(1, 2, dtype=torch.bool), rast, torch.zeros(3, dtype=torch.long), tets, 4),
                 lambda: sv.label_vertices(torch.zeros(1, 2, dtype=torch.bool), rast, torch.zeros(3, dtype=torch.long), tets[:, :3], 5),
                 lambda: sv.label_vertices(torch.zeros(1, 2, dtype=torch.bool), rast, torch.zeros(3, dtype=torch.long), tets, 0),
                 lambda: sv.fit_single_view(geo, {"mvp": mvp}, 1)):
        with pytest.raises(ValueError):
            call()
    big = torch.zeros(1, 1, 2049, 4)
    with pytest.raises(_lib.MeshDiffusionHipError):
        sv.window_min_depth(big)


@pytest.mark.parametrize("radius", (0, 1, 2, 7))
def test_window_minimum_restated_against_a_double_loop(radius):
    rast = vc.hand_rast()
    got = vc.window_min_restated(rast, radius)
    D = vc.corrected_depth(rast)[0]
    want = torch.empty(6, 6)
    for i in range(6):
        for j in range(6):
            want[i, j] = min(float(D[a, b]) for a in range(max(i - radius, 0), min(i + radius, 5) + 1)
                             for b in range(max(j - radius, 0), min(j + radius, 5) + 1))
    assert got.shape == (1, 6, 6) and got.dtype == torch.float32
    assert torch.equal(got[0].view(torch.int32), want.view(torch.int32))       # bit for bit: no -0.0 comes out of the negation
    if radius == 0:
        assert torch.equal(got[0], D) and float(got[0, 0, 0]) == vc.EMPTY and float(got[0, 2, 1]) == -0.125
    if radius == 7:
        assert bool((got == -0.5).all())                                       # every window holds the whole image


def test_visible_tets_restated_against_a_double_loop():
    rast = vc.hand_rast()
    f32 = np.float32
    # mvp = identity: the centres are clip coordinates with w = 1; the grid below lands on and between every pixel and depth step
    g = torch.linspace(-1.25, 1.25, 11)
    centres = torch.stack(torch.meshgrid(g, g, torch.tensor([-1.1, -0.6, -0.125, 0.1, 0.6, 1.0, 1.2]), indexing="ij"), -1).reshape(-1, 3)
    centres = torch.cat([centres, torch.tensor([[float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0]])])
    mvp = torch.eye(4)[None].clone()
    flipped = mvp.clone()
    flipped[0, 3, 3] = -1.0                                                    # w = -1: the contract's deviation
    for radius in (0, 1, 2):
        got = vc.visible_tets_restated(rast, centres, mvp, radius)[0]
        dmin = vc.window_min_restated(rast, radius)[0]
        want = torch.zeros(centres.shape[0], dtype=torch.bool)
        for t, (x, y, z) in enumerate(centres.numpy()):
            q = [np.rint((f32(v) / f32(2) + f32(0.5)) * f32(5)) for v in (x, y, z)]
            if all(0 <= v <= 5 for v in q):
                d = float(dmin[int(q[1]), int(q[0])])
                want[t] = bool(d >= z or d == vc.EMPTY)
        print(f"\nhand-made layer, r = {radius}: {int(want.sum())} of {want.numel()} centres visible")
        assert torch.equal(got, want) and 0 < int(want.sum()) < want.numel()
        assert not bool(vc.visible_tets_restated(rast, centres, flipped, radius).any())
    # labels: two tets per visible flag pattern, hand-checked
    tets = torch.tensor([[0, 1, 2, 3], [2, 3, 4, 5], [5, 6, 7, 8], [8, 9, 10, 11]])
    visible = torch.tensor([[True, False, False, False], [False, False, False, False]])
    face_tet = torch.tensor([2, 2, 1, 0])                                      # ids 1..4 of the layer -> tets 2, 2, 1, 0
    vis, vis_rast = vc.label_vertices_restated(visible, rast.expand(2, 6, 6, 4), face_tet, tets, 13)
    assert vis.dtype == torch.float32 and vis_rast.dtype == torch.bool
    assert vis.tolist() == [1.0] * 4 + [0.0] * 9 and vis_rast.tolist() == [True] * 9 + [False] * 4
    vis, vis_rast = vc.label_vertices_restated(visible, torch.zeros(2, 6, 6, 4), face_tet, tets, 13)
    assert torch.equal(vis.bool(), vis_rast)                                   # nothing rasterised: both labels agree


def test_carve_single_view_truncates_and_runs_anywhere():
    from meshdiffusion_amd import singleview as sv
    H, W = 40, 72
    pos, _ = vc.grid()
    pos = pos[::7].contiguous()
    mvp, _ = rc.cameras(rc.ANGLES, H, W)
    gen = torch.Generator().manual_seed(4)
    mask = (torch.rand(2, H, W, 1, generator=gen) > 0.5).float()
    sdf0 = torch.randn(pos.shape[0], generator=gen) * 1.5
    geo = types.SimpleNamespace(sdf=torch.nn.Parameter(sdf0.clone()), get_deformed=lambda: pos)
    n = sv.carve_single_view(geo, {"mvp": mvp, "mask_cont": mask, "resolution": [H, W]})
    want = vc.carve_single_view_restated(pos, sdf0, mvp, mask, H, W)
    changed = int((want != sdf0).sum())
    print(f"\ncarve on random masks: {n} vertices on empty pixels, {changed} values changed")
    assert torch.equal(geo.sdf.data, want) and 0 < changed <= n < pos.shape[0]
    assert bool((want[want != sdf0] >= 0).all()) and float(want.max()) > 1.0      # untouched positives keep values above 1
    # truncation, not rounding: a vertex at unit coordinate 0.99 of a 2-pixel image lands on pixel 0
    geo = types.SimpleNamespace(sdf=torch.nn.Parameter(torch.tensor([-0.5])), get_deformed=lambda: torch.tensor([[0.98, -1.0, 0.0]]))
    m = torch.tensor([0.0, 1.0]).view(1, 1, 2, 1)
    assert sv.carve_single_view(geo, {"mvp": torch.eye(4)[None], "mask_cont": m, "resolution": [1, 2]}) == 1
    assert float(geo.sdf.data) == 0.5


def test_fixture_holds_only_shares_and_they_are_under_the_cap():
    path = os.path.join(GOLD, "visibility.npz")
    gold = np.load(path)
    assert os.path.getsize(path) < 16 * 1024 and all(gold[k].size == 1 for k in gold.files)
    assert float(gold["init/nn_gap"]) == vc.NN_GAP and float(gold["init/dot_gap"]) == vc.DOT_GAP
    for name in vc.INIT_CASES:
        share, outside = float(gold[f"init/{name}/unsure_share"]), float(gold[f"init/{name}/outside_share"])
        print(f"\ninit_with_gt_surface {name}: ill-conditioned share {share:.5f}, vertices set {outside:.3f}")
        assert 0 <= share <= rc.EXCLUDE_CAP and 0.05 < outside < 0.95


def test_partial_dict_goes_through_cond_gen_scatter(tmp_path, monkeypatch):
    from meshdiffusion_amd.lib.diffusion import evaler
    tet_path = os.path.join(GOLD, "64_tets_cropped.npz")
    verts = torch.tensor(np.load(tet_path)["vertices"])
    N, R = verts.shape[0], 64
    gen = torch.Generator().manual_seed(9)
    partial = {"sdf": torch.sign(torch.randn(N, generator=gen)), "deform": torch.zeros(N, 3),
               "vis": (torch.rand(N, generator=gen) > 0.6).float(), "vis_rast": torch.rand(N, generator=gen) > 0.5}
    path = str(tmp_path / "dmtet.pt")
    torch.save(partial, path)
    idx = evaler.tet_vertices_to_grid_index(verts)
    assert idx.shape == (N, 3) and int(idx.min()) == 0 and int(idx.max()) < R
    assert torch.unique(idx, dim=0).shape[0] == N                              # one cell per vertex: the scatter loses nothing
    seen = {}

    def fake_generate(config, shape_fn, save_fname, run):
        run(None, lambda model, partial, partial_mask, freeze_iters: (seen.update(partial=partial, mask=partial_mask), None)[1:])
        return shape_fn(R)

    monkeypatch.setattr(evaler, "_generate", fake_generate)
    cfg = types.SimpleNamespace(data=types.SimpleNamespace(image_size=R), device="cpu",
                                eval=types.SimpleNamespace(partial_dmtet_path=path, tet_path=tet_path, freeze_iters=3))
    assert evaler.cond_gen(cfg) == (1, 1, R, R, R)
    vis_grid, sdf_grid = seen["mask"], seen["partial"]
    assert vis_grid.shape == (1, 1, R, R, R) and float(vis_grid.sum()) == float(partial["vis"].sum()) > 0
    assert torch.equal(vis_grid[0, 0, idx[:, 0], idx[:, 1], idx[:, 2]], partial["vis"])
    assert torch.equal(sdf_grid[0, 0, idx[:, 0], idx[:, 1], idx[:, 2]], partial["sdf"])
