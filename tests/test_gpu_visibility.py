"""Visible-tet labelling and the single-view fit on the GPU (csrc/visibility.hip, meshdiffusion_amd/singleview.py) against the
restatements of tests/visibility_cases.py.

Bars, none fitted to what the kernels give:
  window_min_depth                  equal to the restatement on the CPU copy of the same `rast`, bit for bit (int32 views).
  visible_tets, vis, vis_rast       torch.equal with the restatement on the CPU: integer decisions on reproducible floats.  No
                                    tolerance, no excluded elements.  Two runs agree bit for bit.
  sphere invariants                 from the geometry, not from the code (see the test).
  carve_single_view                 torch.equal with its restatement.
  init_with_gt_surface              the vertices set to 1.0 are those of the float64 restatement, except where it calls the decision
                                    ill-conditioned in fp32 (the gaps of visibility_cases.py); at most 0.5 % may be left out.
  fit_single_view                   finite terms, a frozen `deform`, a depth term that falls.
Each test prints its figures before it asserts.
"""
import functools
import os

import numpy as np
import pytest
import torch

import raster_cases as rc
import visibility_cases as vc
from conftest import GOLD

pytestmark = pytest.mark.gpu


def _geometry(name, deform=None):
    """A DMTetGeometry of the shipped 64 grid with the case's analytic SDF."""
    from meshdiffusion_amd.dmtet import DMTetGeometry
    geo = DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(rc.case_sdf(name, geo.verts.cpu()).cuda())
        if deform is not None:
            geo.deform.copy_(deform.cuda())
    return geo


@functools.lru_cache(maxsize=None)
def _case(case):
    """The inputs of a grid case, computed once and left unchanged: device tensors and their CPU copies.  The grid is deformed
    (visibility_cases.case_deform), the cameras are raster_cases.cameras(ANGLES): two views."""
    from meshdiffusion_amd import render
    name, H, W = case
    geo = _geometry(name, vc.case_deform(rc.tet_grid()[0].shape[0]))
    with torch.no_grad():
        mesh = geo.getMesh()
        mvp = rc.cameras(rc.ANGLES, H, W)[0].cuda()
        clip = render.xfm_points(mesh.v_pos.detach()[None], mvp).contiguous()
        rast = render.rasterize(clip, mesh.t_pos_idx, (H, W), num_layers=1)[0]
        dev = dict(rast=rast, centres=geo.getTetCenters().detach().contiguous(), mvp=mvp, face_tet=geo.getValidTetIdx(),
                   indices=geo.indices, n_verts=geo.verts.shape[0])
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in dev.items()}
    return dev, cpu


@functools.lru_cache(maxsize=None)
def _restated(case, radius):
    _, c = _case(case)
    visible = vc.visible_tets_restated(c["rast"], c["centres"], c["mvp"], radius)
    return (vc.window_min_restated(c["rast"], radius), visible) + vc.label_vertices_restated(visible, c["rast"], c["face_tet"],
                                                                                           c["indices"], c["n_verts"])


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("radius", vc.RADII)
@pytest.mark.parametrize("case", vc.GRID_CASES, ids=vc.case_id)
def test_labelling_equals_the_restatement(hip_lib, case, radius):
    from meshdiffusion_amd import singleview as sv
    d, c = _case(case)
    want_dmin, want_visible, want_vis, want_vis_rast = _restated(case, radius)
    runs = []
    for _ in range(2):
        dmin = sv.window_min_depth(d["rast"], radius)
        visible = sv.visible_tets(d["rast"], d["centres"], d["mvp"], radius)
        vis, vis_rast = sv.label_vertices(visible, d["rast"], d["face_tet"], d["indices"], d["n_verts"])
        runs.append((dmin, visible, vis, vis_rast))
    dmin, visible, vis, vis_rast = (x.cpu() for x in runs[0])
    covered = int((c["rast"][..., 3] > 0).sum())
    print(f"\n{vc.case_id(case)} r = {radius}: covered pixels {covered} of {c['rast'][..., 3].numel()}, faces {c['face_tet'].shape[0]}, "
          f"window minima differing {int((_bits(dmin) != _bits(want_dmin)).sum())}, visible tets {int(visible.sum())} of "
          f"{visible.numel()} (restated {int(want_visible.sum())}, differing {int((visible != want_visible).sum())}), vis "
          f"{int(vis.sum())} (differing {int((vis != want_vis).sum())}), vis_rast {int(vis_rast.sum())} (differing "
          f"{int((vis_rast != want_vis_rast).sum())})")
    assert dmin.shape == c["rast"].shape[:3] and dmin.dtype == torch.float32
    assert visible.dtype == torch.bool and vis.dtype == torch.float32 and vis_rast.dtype == torch.bool
    assert torch.equal(_bits(dmin), _bits(want_dmin))
    assert torch.equal(visible, want_visible) and torch.equal(vis, want_vis) and torch.equal(vis_rast, want_vis_rast)
    assert 0 < int(visible.sum()) < visible.numel() and covered > 0 and int(vis_rast.sum()) >= int(vis.sum()) > 0
    for a, b in zip(*runs):                                                    # two runs, bit for bit
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else _bits(a), b.view(torch.uint8) if b.dtype == torch.bool else _bits(b))


@pytest.mark.parametrize("radius", vc.RADII)
def test_a_mesh_with_no_faces_hides_nothing(hip_lib, radius):
    from meshdiffusion_amd import singleview as sv
    d, c = _case(("sphere", 40, 72))
    rast = torch.zeros_like(d["rast"])
    visible = sv.visible_tets(rast, d["centres"], d["mvp"], radius)
    valid = vc.project_restated(c["centres"], c["mvp"], 40, 72)[2]
    vis, vis_rast = sv.label_vertices(visible, rast, torch.zeros(0, dtype=torch.long, device="cuda"), d["indices"], d["n_verts"])
    print(f"\nno faces, r = {radius}: valid centres {int(valid.sum())} of {valid.numel()}, visible {int(visible.sum())}")
    assert torch.equal(visible.cpu(), valid) and 0 < int(valid.sum()) < valid.numel()      # some centres leave the 40 x 72 frustum
    assert bool((sv.window_min_depth(rast, radius) == vc.EMPTY).all())
    assert torch.equal(vis.bool(), vis_rast)
    want = vc.label_vertices_restated(valid, torch.zeros_like(c["rast"]), torch.zeros(0, dtype=torch.long), c["indices"], c["n_verts"])
    assert torch.equal(vis.cpu(), want[0]) and torch.equal(vis_rast.cpu(), want[1])


def test_single_view_partial_on_the_sphere(hip_lib):
    """What follows from the geometry: the sphere of radius 0.7 seen from 3 away, 64 x 64, r = 7.
      * A grid vertex with |p| < 0.5: every tet naming it has its vertices within one cell (< 0.06) of it, so its centre lies
        inside the sphere, inside the silhouette and behind the front face at its own pixel, which is in its window: vis = 0.
      * A vertex inside the frustum whose pixel position is more than r + 1 pixels (largest coordinate difference) from every
        covered pixel: the tets around it have centres on every side, one of them no nearer to the silhouette, and its window holds
        no covered pixel: vis = 1.
      * vis_rast >= vis, and every vertex of a tet that owns a face of layer 1 is in vis_rast."""
    from meshdiffusion_amd import render, singleview as sv
    from meshdiffusion_amd.dmtet import DMTetGeometryFixedTopo
    H = W = 64
    r = 7
    geo = _geometry("sphere")
    mvp, campos = rc.cameras((rc.ANGLES[0],), H, W)
    target = {"mvp": mvp.cuda(), "campos": campos.cuda(), "resolution": [H, W]}
    part = sv.single_view_partial(geo, target, radius=r)
    N = geo.verts.shape[0]
    assert set(part) == {"sdf", "deform", "vis", "vis_rast"} and all(not v.is_cuda for v in part.values())
    assert part["vis"].dtype == torch.float32 and part["vis_rast"].dtype == torch.bool and part["sdf"].dtype == torch.float32
    assert part["vis"].shape == part["vis_rast"].shape == part["sdf"].shape == (N,) and part["deform"].shape == (N, 3)
    assert torch.equal(part["sdf"], geo.sdf.detach().cpu()) and bool(((part["vis"] == 0) | (part["vis"] == 1)).all())
    pos = geo.verts.cpu()
    with torch.no_grad():
        mesh = geo.getMesh()
        rast = render.rasterize(render.xfm_points(mesh.v_pos[None], target["mvp"]).contiguous(), mesh.t_pos_idx, (H, W), 1)[0].cpu()
        face_tet = geo.getValidTetIdx().cpu()
    inner = pos.norm(dim=1) < 0.5
    n, _, valid = vc.project_restated(pos, mvp, H, W)
    p = (n[0, :, :2] / 2 + 0.5) * torch.tensor([W - 1, H - 1], dtype=torch.float32)
    ii, jj = torch.nonzero(rast[0, :, :, 3] > 0, as_tuple=True)
    away = torch.maximum((p[:, None, 0] - jj[None].float()).abs(), (p[:, None, 1] - ii[None].float()).abs()).min(1).values
    free = valid[0] & (p >= 0).all(1) & (p[:, 0] <= W - 1) & (p[:, 1] <= H - 1) & (away > r + 1)
    ids = rast[..., 3].unique()
    owners = geo.indices.cpu()[face_tet[ids[ids > 0].long() - 1]].unique()
    vis, vis_rast = part["vis"], part["vis_rast"]
    print(f"\nsphere, one view: vis {int(vis.sum())} vis_rast {int(vis_rast.sum())} of {N}; |p| < 0.5: {int(inner.sum())} vertices, "
          f"{int(vis[inner].sum())} visible; beyond r + 1 pixels of the silhouette: {int(free.sum())} vertices, {int(vis[free].sum())} "
          f"visible; vertices of tets that own a face: {owners.numel()}, {int(vis_rast[owners].sum())} in vis_rast")
    assert int(inner.sum()) > 1000 and not bool(vis[inner].any())
    assert int(free.sum()) > 1000 and bool((vis[free] == 1).all())
    assert bool((vis_rast.float() >= vis).all()) and owners.numel() > 0 and bool(vis_rast[owners].all())
    # two views give the union of the views; the fixed-topology geometry saves its sign, and the geometric invariants hold for
    # its mesh (the crossing edges' midpoints) as well
    mvp2, campos2 = rc.cameras(rc.ANGLES, H, W)
    both = sv.single_view_partial(geo, {"mvp": mvp2.cuda(), "campos": campos2.cuda(), "resolution": [H, W]}, radius=r)
    other = sv.single_view_partial(geo, {"mvp": mvp2[1:].cuda(), "campos": campos2[1:].cuda(), "resolution": [H, W]}, radius=r)
    assert torch.equal(both["vis"], torch.maximum(vis, other["vis"])) and torch.equal(both["vis_rast"], vis_rast | other["vis_rast"])
    fixed = DMTetGeometryFixedTopo(geo, 64, rc.MESH_SCALE, deform_scale=2.0)
    pf = sv.single_view_partial(fixed, target, radius=r)
    assert torch.equal(pf["sdf"], fixed.sdf_sign.detach().cpu()) and bool((pf["sdf"].abs() == 1).all())
    assert pf["vis"].shape == (N,) and not bool(pf["vis"][inner].any()) and bool((pf["vis_rast"].float() >= pf["vis"]).all())


def test_carve_single_view_equals_its_restatement(hip_lib):
    from meshdiffusion_amd import render, singleview as sv
    H, W = 40, 72
    geo = _geometry("torus", vc.case_deform(rc.tet_grid()[0].shape[0]))
    gt_verts, gt_faces = (x.cuda() for x in rc.mesh("sphere"))
    mvp, campos = (x.cuda() for x in rc.cameras(rc.ANGLES, H, W))
    target = render.make_targets(gt_verts, gt_faces, mvp, campos, (H, W))
    sdf0 = geo.sdf.detach().clone() * 3.0                                     # values on both sides of the clamp at 1
    with torch.no_grad():
        geo.sdf.copy_(sdf0)
    n = sv.carve_single_view(geo, target)
    want = vc.carve_single_view_restated(geo.get_deformed().detach(), sdf0, mvp, target["mask_cont"], H, W)
    changed = int((want != sdf0).sum())
    print(f"\ncarve 40 x 72, two views: {n} vertices on empty pixels, {changed} values changed")
    assert torch.equal(geo.sdf.detach(), want) and 0 < changed <= n < sdf0.numel()


@pytest.mark.parametrize("name", vc.INIT_CASES)
def test_init_with_gt_surface_against_float64(hip_lib, name):
    from meshdiffusion_amd import render
    gold = np.load(os.path.join(GOLD, "visibility.npz"))
    geo = _geometry("sphere", vc.case_deform(rc.tet_grid()[0].shape[0]))
    with torch.no_grad():
        geo.sdf.fill_(-0.5)
    gt_verts, gt_faces = (x.cuda() for x in rc.mesh(name))
    mvp, campos = (x.cuda() for x in rc.cameras((vc.INIT_ANGLE,), vc.INIT_RES, vc.INIT_RES))
    seen = render.render_depth(gt_verts, gt_faces, mvp, campos, vc.INIT_RES)["rast_triangle_id"]
    surface = gt_faces[seen]
    n_set = geo.init_with_gt_surface(gt_verts, surface, campos[0])
    got = geo.sdf.detach() == 1.0
    ref = vc.init_with_gt_surface_restated(geo.get_deformed().detach(), gt_verts, surface, campos[0], torch.float64)
    N = got.numel()
    share = float(ref["unsure"].sum()) / N
    wrong = int(((got != ref["outside"]) & ~ref["unsure"]).sum())
    print(f"\ninit_with_gt_surface {name}: visible faces {surface.shape[0]}, set to 1.0 {n_set} (float64 {int(ref['outside'].sum())}), "
          f"differing {int((got != ref['outside']).sum())}, ill-conditioned {int(ref['unsure'].sum())} ({share:.5f}; recorded on the CPU "
          f"{float(gold[f'init/{name}/unsure_share']):.5f}), differing outside that set {wrong}")
    assert share <= rc.EXCLUDE_CAP and float(gold[f"init/{name}/unsure_share"]) <= rc.EXCLUDE_CAP
    assert n_set == int(got.sum()) and 0.05 * N < n_set < 0.95 * N
    assert wrong == 0
    assert bool((geo.sdf.detach()[~got] == -0.5).all()) and geo.sdf.grad is None      # the others untouched; no gradient


def test_tool_writes_the_dict_cond_gen_reads(hip_lib, tmp_path, monkeypatch):
    """tools/fit_singleview.py in this process: `.obj` + one camera -> 12 iterations, 3 of the second pass -> dmtet.pt, and the
    file goes through `evaler.cond_gen`'s load and scatter (its sampler replaced: tests/test_gpu_cli.py runs that)."""
    import sys
    import types
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fit_singleview
    from meshdiffusion_amd import mesh_export
    from meshdiffusion_amd.lib.diffusion import evaler
    gt_verts, gt_faces = rc.mesh("sphere")
    obj, out, tet_path = str(tmp_path / "sphere.obj"), str(tmp_path / "tets" / "dmtet.pt"), os.path.join(GOLD, "64_tets_cropped.npz")
    mesh_export.save_obj(obj, gt_verts, gt_faces)
    fit_singleview.main(["--obj", obj, "--tet_path", tet_path, "--angle", "0.7", "--res", "64", "--iters", "12", "--pass2_iters", "3",
                         "--out", out])
    part = torch.load(out, map_location="cpu", weights_only=False)
    N, R = rc.tet_grid()[0].shape[0], 64
    assert set(part) == {"sdf", "deform", "vis", "vis_rast"} and part["vis"].shape == (N,) and part["deform"].shape == (N, 3)
    assert bool((part["sdf"].abs() == 1).all()) and part["vis_rast"].dtype == torch.bool
    n_vis, n_both = int(part["vis"].sum()), int(part["vis_rast"].sum())
    print(f"\ntools/fit_singleview.py: vis {n_vis} vis_rast {n_both} of {N}")
    assert 0 < n_vis <= n_both < N
    seen = {}

    def fake_generate(config, shape_fn, save_fname, run):
        run(None, lambda model, partial, partial_mask, freeze_iters: (seen.update(partial=partial, mask=partial_mask), None)[1:])

    monkeypatch.setattr(evaler, "_generate", fake_generate)
    evaler.cond_gen(types.SimpleNamespace(data=types.SimpleNamespace(image_size=R), device="cuda",
                                          eval=types.SimpleNamespace(partial_dmtet_path=out, tet_path=tet_path, freeze_iters=3)))
    assert seen["mask"].shape == (1, 1, R, R, R) and float(seen["mask"].sum()) == n_vis
    assert float(seen["partial"].abs().sum()) == N


def test_fit_single_view_thirty_iterations(hip_lib):
    """Measured on MI355X: see the figures this test prints; the bar on the depth term was set before any run."""
    from meshdiffusion_amd import render, singleview as sv
    from meshdiffusion_amd.dmtet import DMTetGeometry
    torch.manual_seed(0)
    geo = DMTetGeometry(64, rc.MESH_SCALE, None, tets=rc.tet_grid(), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(rc.fit_initial_sdf(geo.verts.cpu()).cuda())
    gt_verts, gt_faces = (x.cuda() for x in rc.mesh("sphere"))
    mvp, campos = (x.cuda() for x in rc.cameras((rc.FIT_ANGLES[0],), rc.FIT_RES, rc.FIT_RES))
    target = render.make_targets(gt_verts, gt_faces, mvp, campos, rc.FIT_RES, shaded=True)
    deform0 = geo.deform.detach().clone()
    sdf0 = geo.sdf.detach().clone()
    terms = sv.fit_single_view(geo, target, 30, lr=rc.FIT_LR, sdf_regularizer=rc.FIT_SDF_REGULARIZER, gt_mesh=(gt_verts, gt_faces))
    first, last = float(terms["depth"][:5].mean()), float(terms["depth"][-5:].mean())
    print(f"\nfit_single_view, 30 iterations at 64 x 64: depth {[round(float(x), 4) for x in terms['depth']]}\n  alpha first / last "
          f"{float(terms['alpha'][0]):.5f} / {float(terms['alpha'][-1]):.5f}, colour {float(terms['color'][0]):.5f} / "
          f"{float(terms['color'][-1]):.5f}; depth mean of the first five {first:.5f}, of the last five {last:.5f}; sdf values moved "
          f"{int((geo.sdf.detach() != sdf0).sum())}")
    assert set(terms) == {"depth", "alpha", "color"} and all(v.shape == (30,) and bool(torch.isfinite(v).all()) for v in terms.values())
    assert torch.equal(_bits(geo.deform.detach()), _bits(deform0)) and geo.deform.requires_grad
    assert int((geo.sdf.detach() != sdf0).sum()) > 0
    assert last < first
