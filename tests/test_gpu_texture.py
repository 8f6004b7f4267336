"""Textures on the GPU (meshdiffusion_amd/texture.py, render.render_textured, fit.fit_texture, csrc/texture.hip) against the
restatements of tests/texture_cases.py: the fetch bit for bit against fp32 numpy, its two gradients, the dilation and the projection
bake against float64 at bars recorded by tools/gen_golden_texture.py (4 x the distance of the fp32 restatement from float64), and
the pipeline end to end.

Figures measured on an MI355X are printed by every test (run with -s) and quoted in DESIGN.md section 2, "Textures"."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import texture_cases as tc
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "texture.npz"))


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the fetch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.SAMPLE_CASES, ids=tc.sample_case_id)
def test_forward_is_the_fp32_restatement_bit_for_bit(hip_lib, case):
    from meshdiffusion_amd import texture
    tex, uv, rast, _ = tc.sample_case_inputs(case)
    boundary = case[5]
    want = tc.sample_restated(tex, uv, rast, boundary, np.float32)
    got = texture.sample(_cuda(tex), _cuda(uv), _cuda(rast), boundary).cpu().numpy()
    live = tc.tap(uv, rast, tex.shape[1], tex.shape[2], boundary, np.float32)[0]
    print(f"\n{tc.sample_case_id(case)}: {int(live.sum())} of {live.size} pixels sampled, {int((_bits(got) != _bits(want)).sum())} words differ")
    assert np.array_equal(_bits(got), _bits(want))
    assert not _bits(got[~live]).any() and (live.all() or live.size < 8 or (~live).sum() >= 3)       # skipped: exactly +0
    if tex.shape[0] == 1:                                                       # [Ht,Wt,C] is [1,Ht,Wt,C]
        again = texture.sample(_cuda(tex[0]), _cuda(uv), _cuda(rast), boundary).cpu().numpy()
        assert np.array_equal(_bits(again), _bits(got))


def _backward(texture, t, u, r, g, boundary, plan=None):
    """(out, d tex, d uv) numpy of sum(g * sample) on the device tensors t, u (leaves), r."""
    t.grad = u.grad = None
    out = texture.sample(t, u, r, boundary, plan=plan)
    out.backward(g)
    return out.detach().cpu().numpy(), t.grad.cpu().numpy(), u.grad.cpu().numpy()


@pytest.mark.parametrize("case", tc.BWD_CASES, ids=tc.sample_case_id)
def test_backward_against_float64(hip_lib, gold, case):
    """Bars: 4 x the distance of the fp32 restatement's own gradient from float64 (tests/golden/texture.npz; 0 where the restatement
    is exact); d uv is compared off the kinks (x or y within 1e-4 of an integer, where it jumps).  Two runs and a reused
    SamplePlan give the same bits; texels nobody sampled get exactly 0."""
    from meshdiffusion_amd import texture
    cid = tc.sample_case_id(case)
    tex, uv, rast, G = tc.sample_case_inputs(case)
    boundary = case[5]
    dev = (_cuda(tex).requires_grad_(True), _cuda(uv).requires_grad_(True), _cuda(rast), _cuda(G))
    out1, dtex1, duv1 = _backward(texture, *dev, boundary)
    out2, dtex2, duv2 = _backward(texture, *dev, boundary)
    plan = texture.SamplePlan(dev[1], dev[2], tex.shape, boundary)              # of these very tensors
    out3, dtex3, duv3 = _backward(texture, *dev, boundary, plan)
    out4, dtex4, duv4 = _backward(texture, *dev, boundary, plan)                 # the plan's CSR is built by now
    for a, b in ((out1, out2), (dtex1, dtex2), (duv1, duv2), (out1, out3), (dtex1, dtex3), (duv1, duv3), (dtex1, dtex4), (duv1, duv4)):
        assert np.array_equal(_bits(a), _bits(b))
    want_dtex, want_duv, kink = tc.sample_grads_restated(tex, uv, G, rast, boundary, np.float64)
    err_t, err_u = tc.rel_l2(dtex1, want_dtex), tc.rel_l2(duv1[~kink], want_duv[~kink])
    bar_t, bar_u = tc.bar(gold[f"bwd/{cid}/ref_err_dtex"]), tc.bar(gold[f"bwd/{cid}/ref_err_duv"])
    print(f"\n{cid}: dtex rel-L2 vs float64 {err_t:.2e} (bar {bar_t:.2e}) duv {err_u:.2e} (bar {bar_u:.2e}), {int(kink.sum())} kinks")
    assert np.isfinite(dtex1).all() and np.isfinite(duv1).all()
    T, Ht, Wt, _ = tex.shape
    live, ix0, ix1, iy0, iy1, *_ = tc.tap(uv, rast, Ht, Wt, boundary, np.float32)
    touched = np.zeros((T, Ht, Wt), bool)
    tb = (np.arange(uv.shape[0]) if T > 1 else np.zeros(uv.shape[0], np.int64))[:, None, None] + np.zeros_like(ix0)
    for ix, iy in ((ix0, iy0), (ix1, iy0), (ix0, iy1), (ix1, iy1)):
        touched[tb[live], iy[live], ix[live]] = True
    assert not _bits(dtex1[~touched]).any()                                     # every element is written; nobody's texel: exactly +0
    if case == tc.EXTRA_BWD_CASES[1]:                                           # 9 pixels on 64 x 64 texels
        assert (~touched).sum() >= 64 * 64 - 36
    assert not _bits(duv1[~live]).any()
    assert err_t <= bar_t and err_u <= bar_u


def test_a_plan_of_other_tensors_is_refused(hip_lib):
    from meshdiffusion_amd import texture
    tex, uv, rast, _ = tc.sample_case_inputs(tc.SAMPLE_CASES[6])
    t, u, r = _cuda(tex), _cuda(uv), _cuda(rast)
    plan = texture.SamplePlan(u, r, tex.shape)
    texture.sample(t, u, r, plan=plan)
    for args, kw in (((t, u.clone(), r), {}), ((t, u, r.clone()), {}), ((t, u, None), {}), ((t, u, r), {"boundary": "wrap"}),
                     ((torch.cat([t, t], 2), u, r), {})):
        with pytest.raises(ValueError, match="plan"):
            texture.sample(*args, plan=plan, **kw)
    u.mul_(0.5)                                                                 # written since the plan was built
    with pytest.raises(ValueError, match="plan"):
        texture.sample(t, u, r, plan=plan)


# ---- dilation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.dilate_cases()))
def test_dilate_against_the_restatement(hip_lib, gold, name):
    from meshdiffusion_amd import texture
    tex, mask = tc.dilate_cases()[name]
    want_t, want_m = tex.astype(np.float64), mask
    for steps in (1, 2, 3):
        want_t, want_m = tc.dilate_restated(want_t.astype(np.float32) if steps == 1 else want_t, want_m)
        got_t, got_m = texture.dilate(_cuda(tex), _cuda(mask), steps)
        err = tc.rel_l2(got_t.cpu().numpy(), want_t)
        print(f"\n{name} {steps} steps: covered {int(want_m.sum())} of {want_m.size}, rel-L2 vs float64 {err:.2e} (bar {tc.bar(gold[f'dilate/{name}/ref_err']):.2e})")
        assert np.array_equal(got_m.cpu().numpy(), want_m)
        assert err <= tc.bar(gold[f"dilate/{name}/ref_err"])
    if name in ("empty", "full"):
        assert np.array_equal(_bits(got_t.cpu().numpy()), _bits(tex))


# ---- the projection bake ----------------------------------------------------------------------------------------------------------
def _scene(case):
    """The GPU's own buffers of a baking case: mesh, atlas, render_uv, cameras, position images, depth and mask of every view."""
    from meshdiffusion_amd import render, texture
    name, n_views, side, R = case
    verts, faces = (x.cuda() for x in tc.MESHES[name]())
    uvs, uv_idx = (x.cuda() for x in texture.face_atlas(faces.shape[0], R))
    bake = texture.render_uv(verts, faces, uvs, uv_idx, R)
    mvp, campos = (x.cuda() for x in tc.view_cameras(n_views, side))
    buf = render.render_depth(verts, faces, mvp, campos, side)
    pos = render.interpolate(verts, buf["rast"], faces)
    return dict(verts=verts, faces=faces, uvs=uvs, uv_idx=uv_idx, bake=bake, mvp=mvp, campos=campos, depth=buf["depth"][..., 0],
                viewmask=buf["mask"][..., 0], pos=pos, R=R, side=side)


@pytest.mark.parametrize("case", tc.PROJECT_CASES, ids=tc.project_case_id)
def test_project_views_against_float64_on_the_gpus_own_buffers(hip_lib, gold, case):
    """A texel is left out only where a test of the contract came within 1e-4 of its threshold in float64 (at most 1 % of the masked
    texels); the rest at 4 x the distance of the fp32 restatement from float64."""
    from meshdiffusion_amd import texture
    cid = tc.project_case_id(case)
    s = _scene(case)
    images = tc.smooth_color(s["pos"]) * s["viewmask"][..., None]
    color, weight = texture.project_views(s["bake"], images, s["depth"], s["viewmask"], s["mvp"], s["campos"])
    n = lambda t: t.cpu().numpy()
    want_c, want_w, unsafe = tc.project_restated(n(s["bake"]["pos"]), n(s["bake"]["normal"]), n(s["bake"]["mask"]), n(images), n(s["depth"]),
                                                 n(s["viewmask"]), n(s["mvp"]), n(s["campos"]))
    on = n(s["bake"]["mask"]) > 0.5
    keep = on & ~unsafe
    left_out = float((unsafe & on).sum() / on.sum())
    got_c, got_w = n(color), n(weight)
    err_c, err_w = tc.rel_l2(got_c[keep], want_c[keep]), tc.rel_l2(got_w[keep], want_w[keep])
    bar_c, bar_w = tc.bar(gold[f"project/{cid}/ref_err_color"]), tc.bar(gold[f"project/{cid}/ref_err_weight"])
    print(f"\n{cid}: masked {int(on.sum())} seen {int((want_w > 0).sum())} left out {left_out:.4f} (CPU buffers: "
          f"{float(gold[f'project/{cid}/left_out']):.4f}); colour rel-L2 {err_c:.2e} (bar {bar_c:.2e}) weight {err_w:.2e} (bar {bar_w:.2e})")
    assert left_out <= tc.MAX_LEFT_OUT and (want_w > 0).sum() > 0.5 * on.sum()
    assert not got_c[~on].any() and not got_w[~on].any()
    assert np.array_equal(got_w[keep] > 0, want_w[keep] > 0)
    assert err_c <= bar_c and err_w <= bar_w


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def round_trip(hip_lib):
    """The scene of the round trip, computed once: T0, its eight renders (raw kd, no antialiasing), the bake T1."""
    from meshdiffusion_amd import render, texture
    s = _scene(tc.ROUND_TRIP)
    bake = s["bake"]
    t0 = torch.where(bake["mask"][..., None] > 0.5, tc.smooth_color(bake["pos"]), torch.full_like(bake["pos"], 0.5))
    t0 = texture.dilate(t0, bake["mask"], 1)[0]
    with torch.no_grad():
        img = render.render_textured(s["verts"], s["faces"], s["uvs"], s["uv_idx"], t0, s["mvp"], s["campos"], s["side"], shade=False,
                                     antialias=False)
    baked = texture.bake_from_views(s["verts"], s["faces"], img[..., :3].contiguous(), img[..., 3], s["mvp"], s["campos"], s["R"])
    s.update(t0=t0, images=img[..., :3].contiguous(), alpha=img[..., 3].contiguous(), baked=baked)
    return s


def test_round_trip_render_then_bake(round_trip, gold):
    s = round_trip
    assert torch.equal(s["baked"]["uvs"], s["uvs"]) and torch.equal(s["baked"]["uv_idx"], s["uv_idx"])
    assert torch.equal(s["alpha"], s["viewmask"])
    seen = s["baked"]["weight"] > 0
    err = (s["baked"]["tex"] - s["t0"]).abs()[seen]
    bar = 1.5 * float(gold["round_trip/cpu_err"])
    print(f"\nround trip {tc.project_case_id(tc.ROUND_TRIP)}: seen {float(seen.sum() / (s['bake']['mask'] > 0.5).sum()):.3f} of the masked "
          f"texels, |T1 - T0| max {float(err.max()):.4f} mean {float(err.mean()):.5f} (CPU pipeline: max {float(gold['round_trip/cpu_err']):.4f} "
          f"mean {float(gold['round_trip/cpu_mean_err']):.5f}; bar {bar:.4f})")
    assert float(seen.sum()) > 0.9 * float((s["bake"]["mask"] > 0.5).sum())
    assert float(err.max()) <= bar
    assert float(err.mean()) <= 1.5 * float(gold["round_trip/cpu_mean_err"])     # a half-texel or orientation error would show here
    unseen = (s["bake"]["mask"] > 0.5) & ~seen
    assert bool((s["baked"]["tex"][unseen] == 0.5).all())                         # fill


def test_fit_texture_lowers_the_loss_from_the_bake(round_trip):
    from meshdiffusion_amd import fit
    s = round_trip
    targets = {"images": s["images"], "viewmask": s["alpha"], "mvp": s["mvp"], "campos": s["campos"]}
    tex, hist = fit.fit_texture(s["verts"], s["faces"], s["uvs"], s["uv_idx"], targets, s["R"], 30, lr=2e-4, init=s["baked"]["tex"], shade=False)
    loss = hist["loss"].cpu().numpy()
    print(f"\nfit_texture from the bake: loss {loss[0]:.6f} -> {loss[-1]:.6f} (ratio {loss[-1] / loss[0]:.3f}), largest {loss.max():.6f}")
    assert tuple(tex.shape) == (s["R"], s["R"], 3) and loss.shape == (30,) and np.isfinite(loss).all()
    assert loss[-1] < loss[0] and loss.max() <= 2 * loss[0]                     # never above the start by more than its first value
    tex2, hist2 = fit.fit_texture(s["verts"], s["faces"], s["uvs"], s["uv_idx"], targets, s["R"], 3, lr=2e-4, init=s["baked"]["tex"], shade=False)
    assert np.array_equal(_bits(hist2["loss"].cpu().numpy()), _bits(loss[:3]))  # deterministic


def _interior(mask):
    """Pixels whose 3 x 3 neighbourhood is covered: [B,H,W] bool."""
    m = mask[:, None].float()
    return (-torch.nn.functional.max_pool2d(-m, 3, 1, 1))[:, 0] > 0.5


def test_per_tet_atlas_and_face_atlas_are_interchangeable(hip_lib, gold):
    """One marching-tets mesh (11064 faces), the same position function baked into the per-tet atlas of DMTet() at 2048 and into
    face_atlas at 512: the two textured renders agree within the round-trip bar on interior pixels.  Interior: the pixel and its
    eight neighbours are covered, and in both atlases the four texels of its bilinear footprint were baked from the pixel's own
    face.  The second condition is what the per-tet atlas needs at 2048: its tiles are 5.12 texels with half a texel between them,
    so a fetch near a triangle's border mixes in texels of the neighbouring tile, another tet anywhere on the surface (the reason
    `face_atlas` exists).  Measured on an MI355X over all 4424 covered-neighbourhood pixels, against the colour of the pixel's own
    surface point: per-tet atlas max 0.419 (9 pixels above the bar), face atlas max 0.095; on the 710 interior pixels both 1e-4."""
    import raster_cases as rc
    from meshdiffusion_amd import dmtet, render, texture
    tv, ti = rc.tet_grid()
    pos = torch.as_tensor(tv, dtype=torch.float32).cuda() * rc.MESH_SCALE
    tets = torch.as_tensor(ti, dtype=torch.int64).cuda()
    verts, faces, uvs_tet, idx_tet, *_ = dmtet.DMTet()(pos, rc.case_sdf("sphere", pos.cpu()).cuda(), tets)
    uvs_face, idx_face = (x.cuda() for x in texture.face_atlas(faces.shape[0], 512))
    mvp, campos = (x.cuda() for x in tc.view_cameras(2, 96))
    rast = render.rasterize(render.xfm_points(verts[None], mvp).contiguous(), faces, 96, num_layers=1)[0]
    pix_face = (rast[..., 3].long() - 1).cpu().numpy()
    imgs, own = [], np.ones(pix_face.shape, bool)
    for uvs, idx, R in ((uvs_tet, idx_tet, 2048), (uvs_face, idx_face, 512)):
        bake = texture.render_uv(verts, faces, uvs, idx, R)
        t = torch.where(bake["mask"][..., None] > 0.5, tc.smooth_color(bake["pos"]), torch.full_like(bake["pos"], 0.5))
        t = texture.dilate(t, bake["mask"], 1)[0]
        with torch.no_grad():
            imgs.append(render.render_textured(verts, faces, uvs, idx, t, mvp, campos, 96, shade=False, antialias=False))
        uv = render.interpolate(uvs, rast, idx).cpu().numpy()
        _, ix0, ix1, iy0, iy1, *_ = tc.tap(uv, None, R, R, "clamp", np.float32)
        fid = bake["face_id"].cpu().numpy()
        for ix, iy in ((ix0, iy0), (ix1, iy0), (ix0, iy1), (ix1, iy1)):
            own &= fid[iy, ix] == pix_face
        print(f"\natlas {R}: {int(bake['mask'].sum())} texels covered, {int(torch.unique(bake['face_id']).numel()) - 1} of {faces.shape[0]} faces own a texel")
    covered = _interior(imgs[0][..., 3])
    inside = covered & torch.from_numpy(own).cuda()
    diff = (imgs[0][..., :3] - imgs[1][..., :3]).abs()
    bar = 1.5 * float(gold["round_trip/cpu_err"])
    print(f"per-tet atlas vs face atlas: {int(inside.sum())} interior pixels of {int(covered.sum())} with a covered neighbourhood, max "
          f"difference {float(diff[inside].max()):.4f} mean {float(diff[inside].mean()):.5f} (bar {bar:.4f}); over the covered "
          f"neighbourhoods max {float(diff[covered].max()):.4f} mean {float(diff[covered].mean()):.5f}")
    # the share kept guards the definition itself: measured 710 of 4424 (0.16); an interior set that shrinks is a finding
    assert torch.equal(imgs[0][..., 3], imgs[1][..., 3]) and int(inside.sum()) >= 0.12 * int(covered.sum()) > 400
    assert float(diff[inside].max()) <= bar


def test_texture_from_views_tool(round_trip, gold, tmp_path):
    """The tool on the round-trip scene.  The preview is compared with the target view on pixels whose 3 x 3 neighbourhood is
    covered: the targets are rendered without antialiasing, as the CPU pipeline that sets the bar renders them, and the tool's
    preview is antialiased, so the silhouette ring differs by construction.  (Without antialiasing the CPU pipeline puts the whole
    view at max 0.23 .. 0.27, two or three pixels a view above the bar: texels at the sphere's poles, which every camera sees so
    obliquely that the depth at the nearest pixel lies more than depth_bias in front of them, keep `fill`.)"""
    from meshdiffusion_amd import mesh_export
    s = round_trip
    mesh_export.save_obj(str(tmp_path / "in.obj"), s["verts"], s["faces"], decimal_places=8)
    np.savez(tmp_path / "views.npz", images=s["images"].cpu().numpy(), viewmask=s["alpha"].cpu().numpy(), mvp=s["mvp"].cpu().numpy(),
             campos=s["campos"].cpu().numpy())
    spec = importlib.util.spec_from_file_location("texture_from_views", os.path.join(ROOT, "tools", "texture_from_views.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "out"
    tool.main(["--obj", str(tmp_path / "in.obj"), "--views", str(tmp_path / "views.npz"), "--res", str(s["R"]), "--unshaded", "--out", str(out)])
    for name in ("mesh.obj", "mesh.mtl", "mesh_kd.png", "preview.png"):
        assert os.path.getsize(out / name) > 0, name
    tex = mesh_export.load_png(str(out / "mesh_kd.png"))
    assert tex.shape == (s["R"], s["R"], 3)
    preview = torch.from_numpy(mesh_export.load_png(str(out / "preview.png")).astype(np.float32) / 255).cuda()
    inside = _interior(s["alpha"][:1])[0]
    diff = (preview - s["images"][0]).abs()[inside]
    bar = 1.5 * float(gold["round_trip/cpu_err"])
    print(f"\ntexture_from_views: preview vs target view on {int(inside.sum())} interior pixels: max {float(diff.max()):.4f} mean {float(diff.mean()):.5f} (bar {bar:.4f})")
    assert float(diff.max()) <= bar
