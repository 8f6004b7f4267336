"""The mesh post-processing on the GPU (csrc/meshpost.hip, meshdiffusion_amd/postprocess.py, render.shade_diffuse,
render.render_preview, python -m meshdiffusion_amd.mesh_export) against the restatements of tests/meshpost_cases.py.

Bars, none fitted to what the kernels give:
  components, drop_floaters   torch.equal with the restatement (scipy's connected components, canonicalised).
  smoothing, shading          rel-L2 against the float64 restatement <= 4 x the fp32 torch restatement's OWN rel-L2 distance from
                    float64 for that case, recorded in tests/golden/meshpost.npz by tools/gen_golden_meshpost.py (the margin of
                    tests/test_gpu_fixedtopo.py and tests/test_gpu_interp.py).  Discrete parts are exact: steps = 0, vertices
                    without a row, two runs, the batched form against its halves, alpha, uncovered pixels.
  render_preview    torch.equal with its public pieces composed by hand; a uniform white light renders srgb(kd) within 1e-5.
Each test prints its figures before it asserts.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import interp_cases as ic
import meshpost_cases as mc
import raster_cases as rc
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu
MARGIN = 4.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "meshpost.npz"))


@functools.lru_cache(maxsize=None)
def _gpu_mesh(name):
    v, f = mc.mesh(name)
    return v.cuda(), f.cuda()


@functools.lru_cache(maxsize=None)
def _rows(name):
    v, f = mc.mesh(name)
    return mc.smoothing_rows(f, v.shape[0])


# ---- components ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.CASES)
def test_components_against_the_restatement(hip_lib, name):
    from meshdiffusion_amd import postprocess
    v, f = _gpu_mesh(name)
    V = v.shape[0]
    want_label, want_cf = mc.components_restated(f.cpu(), V)
    runs = [postprocess.components(f, V) for _ in range(2)]
    label, cf, rounds = runs[0]
    print(f"\ncomponents {name}: V {V} F {f.shape[0]} components {int((want_label == np.arange(V)).sum())} rounds {rounds} / "
          f"{runs[1][2]} (synchronous model {mc.rounds_simulated(f.cpu(), V)[1]}), labels differing {int((label.cpu().numpy() != want_label).sum())}")
    assert label.dtype == cf.dtype == torch.int32 and label.shape == cf.shape == (V,)
    assert torch.equal(label.cpu(), torch.as_tensor(want_label)) and torch.equal(cf.cpu(), torch.as_tensor(want_cf))
    assert 1 <= rounds <= mc.MAX_ROUNDS and runs[1][2] <= mc.MAX_ROUNDS
    assert torch.equal(label, runs[1][0]) and torch.equal(cf, runs[1][1])
    if name == "degen":
        assert label.tolist() == mc.DEGEN_LABELS


DROP_SETTINGS = (("degen", dict(keep_largest=True), False), ("noise", dict(keep_largest=True), False),
                 ("degen", dict(min_faces=2), False), ("noise", dict(min_faces=8), False), ("pair", dict(min_faces=8), False),
                 ("noise", dict(min_fraction=0.01), False), ("pair", dict(keep_largest=True), True),
                 ("pair", dict(keep_largest=True), False))


@pytest.mark.parametrize("name,kw,with_mesh", DROP_SETTINGS, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in kw.items())}{'-vm' if m else ''}"
                                                                    for n, kw, m in DROP_SETTINGS])
def test_drop_floaters_against_the_restatement(hip_lib, name, kw, with_mesh):
    from meshdiffusion_amd import postprocess
    v, f = _gpu_mesh(name)
    vm = mc.vert_mesh(name) if with_mesh else None
    want = mc.drop_floaters_restated(v.cpu().numpy(), f.cpu().numpy(), vert_mesh=None if vm is None else vm.numpy(), **kw)
    got = postprocess.drop_floaters(v, f, vert_mesh=None if vm is None else vm.cuda(), **kw)
    left = len(np.unique(mc.components_restated(want[1], want[0].shape[0])[0])) if want[0].shape[0] else 0
    print(f"\ndrop_floaters {name} {kw}{' per mesh' if with_mesh else ''}: {want[0].shape[0]} of {v.shape[0]} vertices, "
          f"{want[1].shape[0]} of {f.shape[0]} faces, {left} components left")
    assert got[0].dtype == torch.float32 and got[1].dtype == got[2].dtype == torch.int64 and got[3].dtype == torch.bool
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), torch.as_tensor(w))
    if with_mesh:
        assert left == 2                                                 # one component per mesh survives
    if name == "noise" and "min_fraction" in kw:
        assert left == 1
    assert torch.equal(_gpu_mesh(name)[0].cpu(), mc.mesh(name)[0])       # the inputs are left as they were


# ---- smoothing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", mc.SMOOTH_SETTINGS, ids=[s[0] for s in mc.SMOOTH_SETTINGS])
@pytest.mark.parametrize("name", mc.CASES)
def test_smoothing_against_float64(hip_lib, gold, name, setting):
    from meshdiffusion_amd import postprocess
    tag, steps, lam, mu = setting
    v, f = _gpu_mesh(name)
    before = v.clone()
    x64 = mc.smooth_restated(v.cpu(), f.cpu(), steps, lam, mu, torch.float64, _rows(name))
    edges = postprocess.mesh_edges(f, v.shape[0])
    runs = [postprocess.smooth(v, f, steps, lam, mu), postprocess.smooth(v, f, steps, lam, mu, edges=edges)]
    e, unit = rc.rel_l2(runs[0], x64), float(gold[f"smooth/{name}/{tag}/ref_err"])
    print(f"\nsmooth {name} {tag}: V {v.shape[0]} rel-L2 vs float64 / unit {e:.2e}/{unit:.2e}={e / unit:.2f}; moved "
          f"{float((runs[0] - v).norm() / v.norm()):.3e} of |x|")
    assert runs[0].dtype == torch.float32 and runs[0].shape == v.shape and runs[0].data_ptr() != v.data_ptr()
    assert torch.equal(runs[0], runs[1])                                 # two runs, bit for bit; the prebuilt table changes nothing
    assert torch.equal(v, before)                                        # the input is never written
    n = torch.as_tensor(_rows(name)[1])
    assert torch.equal(runs[0].cpu()[n == 0], v.cpu()[n == 0])           # a vertex without a row keeps its bits
    if name == "degen":
        assert int((n == 0).sum()) == 1 and torch.equal(runs[0][4], v[4])
    assert e <= MARGIN * unit


@pytest.mark.parametrize("name", mc.CASES)
def test_smoothing_exact_parts(hip_lib, name):
    from meshdiffusion_amd import postprocess
    v, f = _gpu_mesh(name)
    before = v.clone()
    lo, hi, mult, ptr, adj = postprocess.mesh_edges(f, v.shape[0])
    want = mc.edges_restated(f.cpu(), v.shape[0])
    print(f"\nedges {name}: E {lo.shape[0]} boundary {int((mult == 1).sum())} of three or more faces {int((mult >= 3).sum())}")
    for g, w in zip((lo, hi, mult, ptr, adj), want):
        assert torch.equal(g.cpu(), torch.as_tensor(w)) and g.dtype == torch.as_tensor(w).dtype
    zero = postprocess.smooth(v, f, 0)
    assert torch.equal(zero, v) and zero.data_ptr() != v.data_ptr() and torch.equal(v, before)     # steps = 0 copies
    one_three = postprocess.smooth(postprocess.smooth(v, f, 1), f, 2)                               # lam | lam | lam either way
    assert torch.equal(one_three, postprocess.smooth(v, f, 3))


def test_call_helper_passes_tensors_none_and_the_status(hip_lib):
    """hip_ops.call, the one way the mesh-side modules reach an export: a tensor goes as its address, None as null (`scratch`, unused
    with one step), the stream last; a refusal (n_verts = 0, before any launch) raises with the export's name and its code."""
    from meshdiffusion_amd import _lib, postprocess
    from meshdiffusion_amd.hip_ops import call
    v, f = _gpu_mesh("quad")
    ptr, adj = postprocess.mesh_edges(f, v.shape[0])[3:]
    out = torch.full_like(v, float("nan"))
    call("md_mesh_smooth", v, ptr, adj, v.shape[0], adj.numel(), 1, 0.5, float("nan"), out, None)
    assert torch.equal(out, postprocess.smooth(v, f, 1))
    with pytest.raises(_lib.MeshDiffusionHipError) as err:
        call("md_mesh_smooth", v, ptr, adj, 0, adj.numel(), 1, 0.5, float("nan"), out, None)
    print(f"\ncall: {err.value}")
    assert "md_mesh_smooth" in str(err.value) and "-1" in str(err.value)


def test_the_batched_form_equals_its_halves(hip_lib):
    from meshdiffusion_amd import postprocess
    pv, pf = _gpu_mesh("pair")
    halves = [_gpu_mesh("ptorus"), _gpu_mesh("fan40")]
    for tag, steps, lam, mu in mc.SMOOTH_SETTINGS:
        both = postprocess.smooth(pv, pf, steps, lam, mu)
        alone = torch.cat([postprocess.smooth(v, f, steps, lam, mu) for v, f in halves])
        print(f"\npair {tag}: elements differing from the halves done alone {int((both != alone).sum())}")
        assert torch.equal(both, alone)
    out = postprocess.postprocess(halves, smooth_steps=3, keep_largest=True)
    assert len(out) == 2
    for (v, f), (ov, of) in zip(halves, out):
        assert torch.equal(ov, postprocess.smooth(v, f, 3)) and torch.equal(of, f)
    cv, cf, vm = postprocess.concat_meshes(halves)
    assert torch.equal(cv, pv) and torch.equal(cf, pf) and torch.equal(vm.cpu(), mc.vert_mesh("pair"))
    same = postprocess.postprocess(halves)                               # every keyword at its default: nothing happens
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(same, halves))


# ---- shading -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light", mc.LIGHTS)
@pytest.mark.parametrize("case", mc.SHADE_CASES, ids=ic.case_id)
def test_shading_against_float64(hip_lib, gold, case, light):
    from meshdiffusion_amd import render
    verts, faces, mvp, campos, pc, H, W, _ = mc.shade_inputs(case)
    sh, kd = mc.case_light(light)
    rast = render.rasterize(pc.cuda(), faces.cuda(), (H, W), num_layers=1)[0]
    runs = [render.shade_diffuse(rast, verts.cuda(), faces.cuda(), campos.cuda(), sh.cuda(), kd.cuda()) for _ in range(2)]
    got = runs[0].cpu()
    want, gv, cov = mc.shade_restated(rast.cpu(), verts, faces, campos, sh, kd, torch.float64)
    e, unit = mc.rgb_rel_l2(got, want, cov), float(gold[f"shade/{ic.case_id(case)}/{light}/ref_err"])
    margin = float(gv[cov].abs().min())
    front = [int(((gv > 0) & cov)[b].sum()) for b in range(gv.shape[0])]
    print(f"\nshade {ic.case_id(case)} {light}: covered {int(cov.sum())} (front per view {front} of {[int(cov[b].sum()) for b in range(gv.shape[0])]}), "
          f"smallest |geo . view| {margin:.4f}, rgb {float(want[..., :3][cov].min()):.3f}-{float(want[..., :3][cov].max()):.3f}, "
          f"rel-L2 vs float64 / unit {e:.2e}/{unit:.2e}={e / unit:.2f}")
    assert margin >= ic.FLIP_MARGIN                                      # a condition of the test: no pixel sits on the flip
    assert got.shape == (mvp.shape[0], H, W, 4) and got.dtype == torch.float32 and torch.equal(runs[0], runs[1])
    assert bool((got[..., 3][cov] == 1).all()) and not bool(got[~cov].any())     # alpha exactly 1 or 0, uncovered exactly 0
    if case[0] in ("quad", "fan40"):                                     # front in view 0, wholly from behind in view 1
        assert front[0] == int(cov[0].sum()) > 0 and front[1] == 0 < int(cov[1].sum())
    assert e <= MARGIN * unit


def test_shading_ignores_ids_above_the_face_count(hip_lib):
    from meshdiffusion_amd import render
    verts, faces, mvp, campos, pc, H, W, _ = mc.shade_inputs(("quad", 16, 16))
    sh, kd = mc.case_light("random")
    rast = render.rasterize(pc.cuda(), faces.cuda(), (H, W), num_layers=1)[0]
    full = render.shade_diffuse(rast, verts.cuda(), faces.cuda(), campos.cuda(), sh.cuda(), kd.cuda())
    first = render.shade_diffuse(rast, verts.cuda(), faces[:1].cuda(), campos.cuda(), sh.cuda(), kd.cuda())      # id 2 is above F = 1
    is_one = (rast[..., 3] == 1)[..., None]
    assert bool((rast[..., 3] == 2).any()) and torch.equal(first, torch.where(is_one, full, torch.zeros_like(full)))
    none = render.shade_diffuse(rast, verts.cuda(), faces[:0].cuda(), campos.cuda(), sh.cuda(), kd.cuda())
    assert not bool(none.any())


# ---- the preview ---------------------------------------------------------------------------------------------------------------------
def _srgb(f):
    return torch.where(f > 0.0031308, torch.pow(torch.clamp(f, min=0.0031308), 1.0 / 2.4) * 1.055 - 0.055, 12.92 * f)


@pytest.mark.parametrize("antialias", (True, False))
def test_render_preview_is_its_public_pieces(hip_lib, antialias):
    from meshdiffusion_amd import render
    v, f = _gpu_mesh("ptorus")
    res = (40, 72)
    mvp = torch.cat([render.preview_camera(k, res, device="cuda")[0] for k in (0, 9)])
    campos = torch.cat([render.preview_camera(k, res, device="cuda")[1] for k in (0, 9)])
    bg = (0.2, 0.5, 1.0)
    img = render.render_preview(v, f, mvp, campos, res, background=bg, antialias=antialias)
    clip = render.xfm_points(v[None], mvp).contiguous()
    rast = render.rasterize(clip, f, res, num_layers=1)[0]
    col = render.shade_diffuse(rast, v, f, campos, render.default_light(), render.PREVIEW_KD)
    if antialias:
        col = render.antialias(col, rast, clip, f)
    rgb = col[..., :3] + (1 - col[..., 3:]) * torch.tensor(bg, device="cuda")
    want = torch.clamp(_srgb(rgb), 0, 1)
    cov = rast[..., 3] > 0
    print(f"\npreview antialias={antialias}: covered {int(cov.sum())} of {cov.numel()} pixels, range {float(img.min()):.3f}-{float(img.max()):.3f}, "
          f"pixels differing from the pieces {int((img != want).any(-1).sum())}")
    assert img.shape == (2, 40, 72, 3) and img.dtype == torch.float32 and torch.equal(img, want)
    assert float(img.min()) >= 0 and float(img.max()) <= 1 and int(cov.sum()) > 100
    far = ~ic.dilate(cov)                                                # away from the silhouette: the background itself
    assert torch.equal(img[far], torch.clamp(_srgb(torch.tensor(bg, device="cuda")), 0, 1).expand_as(img)[far])


def test_render_preview_empty_mesh_and_white_light(hip_lib):
    from meshdiffusion_amd import render
    v, f = _gpu_mesh("ptorus")
    mvp, campos = render.preview_camera(3, 64, device="cuda")
    bg = torch.tensor((1.0, 0.25, 0.0), device="cuda")
    for ev, ef in ((v[:0], f[:0]), (v, f[:0])):
        img = render.render_preview(ev, ef, mvp, campos, 64, background=tuple(bg.tolist()))
        assert img.shape == (1, 64, 64, 3) and torch.equal(img, torch.clamp(_srgb(bg), 0, 1).expand(1, 64, 64, 3))
    white = torch.zeros(9, 3)
    white[0] = 1 / 0.282095                                               # a uniform environment of radiance 1
    kd = render.PREVIEW_KD
    img = render.render_preview(v, f, mvp, campos, 64, kd=kd, light=white)
    rast = render.rasterize(render.xfm_points(v[None], mvp).contiguous(), f, 64, num_layers=1)[0]
    cov = rast[..., 3] > 0
    interior = cov & ~ic.dilate(~cov)                                     # a covered pixel whose four neighbours are covered
    want = torch.as_tensor(mc.srgb(np.array(kd)), dtype=torch.float32, device="cuda")
    err = float((img[interior] - want).abs().max())
    print(f"\nwhite light: interior covered pixels {int(interior.sum())} of {int(cov.sum())}, max |pixel - srgb(kd)| {err:.2e}")
    assert int(interior.sum()) > 100 and err <= 1e-5


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_command_line_cleans_and_renders(hip_lib, tmp_path):
    from meshdiffusion_amd import mesh_export
    samples = mc.sphere_and_blob_samples()
    np.save(tmp_path / "samples.npy", samples)
    tet = os.path.join(GOLD, "64_tets_cropped.npz")
    base = [sys.executable, "-m", "meshdiffusion_amd.mesh_export", "--sample_path", str(tmp_path / "samples.npy"), "--tet_path", tet]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for out, extra in (("plain", []), ("clean", ["--num_smooth_steps", "3", "--keep_largest", "--preview_dir", str(tmp_path / "png")])):
        r = subprocess.run(base + ["--out", str(tmp_path / out)] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        print(r.stdout[-500:], r.stderr[-2000:])
        assert r.returncode == 0
    t = np.load(tet)
    today = mesh_export.samples_to_obj(samples, t["vertices"], t["indices"], str(tmp_path / "api"))
    for k, path in enumerate(today):
        name = os.path.basename(path)
        assert name == f"{k:06d}.obj"
        raw = open(path, "rb").read()
        assert raw == open(tmp_path / "plain" / name, "rb").read()       # without the new flags: byte-identical to today's
        v0, f0 = mesh_export.load_obj(path)
        v1, f1 = mesh_export.load_obj(str(tmp_path / "clean" / name))
        n0 = len(np.unique(mc.components_restated(f0, v0.shape[0])[0]))
        n1 = len(np.unique(mc.components_restated(f1, v1.shape[0])[0]))
        img = mesh_export.load_png(str(tmp_path / "png" / f"{k:06d}.png"))
        not_bg = int((img != 255).any(-1).sum())
        print(f"mesh {k}: raw {v0.shape[0]} vertices {f0.shape[0]} faces {n0} components; cleaned {v1.shape[0]} / {f1.shape[0]} / {n1}; "
              f"preview {img.shape} pixels off the background {not_bg}")
        assert n0 == 2 and n1 == 1 and 0 < f1.shape[0] < f0.shape[0]
        assert img.shape == (512, 512, 3) and img.dtype == np.uint8 and not_bg > 1000
    assert len(today) == 2 and sorted(os.listdir(tmp_path / "png")) == ["000000.png", "000001.png"]
