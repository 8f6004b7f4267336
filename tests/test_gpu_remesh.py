"""Isotropic remeshing on the GPU (csrc/remesh.hip, meshdiffusion_amd/postprocess.py remesh, python -m meshdiffusion_amd.mesh_export
--remesh_iters) against the float32 numpy restatement of tests/remesh_cases.py.

Bars, none fitted to what the kernels give:
  split, a collapse round, a flip round, the whole pipeline without relax    faces torch.equal and verts bit-equal with the
                    restatement from the same state (midpoints and copies are the only arithmetic), winner counts equal.
  relax             rel-L2 against the float64 restatement <= 4 x the float32 restatement's OWN rel-L2 distance from float64,
                    recorded in tests/golden/remesh.npz by tools/gen_golden_remesh.py (the margin of tests/test_gpu_meshpost.py);
                    fixed vertices bit-unchanged.
  with relax on     conditions by construction: a valid closed orientable manifold of the same Euler characteristic, boundary
                    vertices untouched, the batch equal to its halves, two runs equal.  Quality (5 iterations, as the prototype
                    behind the scheme): the band share and the minimum angle after strictly above those before; fidelity on the
                    unit sphere: max | |x| - 1 | <= 2 x the restatement's recorded value.
Each test prints its figures before it asserts.

Figures of the restatement (tools/gen_golden_remesh.py; the kernels reproduce its decisions): uvsphere x 1.0 share 0.697 -> 0.947,
minimum angle 14.0 -> 37.1; x 0.6 0.121 -> 0.951, 14.0 -> 34.1; ptorus x 1.0 share 0.333 -> 0.975, minimum angle 31.0 -> 41.6; x 0.6
0.458 -> 0.856, 31.0 -> 34.9.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshpost_cases as mc
import raster_cases as rc
import remesh_cases as rm
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu
MARGIN = 4.0
RELAX = 0.5


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "remesh.npz"))


def _dev(*arrays):
    return tuple(torch.as_tensor(np.ascontiguousarray(a)).cuda() for a in arrays)


def _same(got, want):
    """bit-equal floats or equal integers, shapes included"""
    w = torch.as_tensor(want)
    g = got.cpu()
    return g.shape == w.shape and (torch.equal(g.view(torch.int32), w.view(torch.int32)) if w.dtype == torch.float32 else torch.equal(g, w.to(g.dtype)))


@functools.lru_cache(maxsize=None)
def _run(name, scale=1.0, relax=RELAX, iters=rm.PIPELINE_ITERS):
    from meshdiffusion_amd import postprocess
    v, f = rm.mesh(name)
    return postprocess.remesh(v.cuda(), f.cuda(), iters=iters, target_scale=scale, relax=relax, vert_mesh=rm.vert_mesh(name).cuda())


def _rounds(info):
    return [tuple(r.values()) for r in info["iterations"]]


# ---- 1: every pass from the restatement's state ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rm.EXACT_CASES)
def test_each_pass_equals_the_restatement(hip_lib, gold, name):
    from meshdiffusion_amd import postprocess
    s0, s1, s2, s3 = rm.pass_states(name)
    target, lo2, hi2 = rm.case_bands(name)
    got_target = postprocess.remesh_default_target(*_dev(s0[0], s0[1], s0[2]), target.shape[0])
    dlo2, dhi2 = _dev(lo2, hi2)
    x, f, vm = _dev(*s0[:3])
    g1 = postprocess.remesh_split(x, f, vm, dhi2)
    x, f, vm = _dev(*s1[:3])
    before = x.clone()
    g2 = postprocess.remesh_collapse_round(x, f, vm, dlo2, dhi2)
    x, f, vm = _dev(*s2[:3])
    g3 = postprocess.remesh_flip_round(x, f, float(rm.cos2_of(30.0)))
    print(f"\n{name}: target {target.tolist()} (device {got_target.tolist()}); split {g1[3]} / {s1[3]} marked, F {s0[1].shape[0]} -> "
          f"{g1[1].shape[0]}; collapse round {g2[3]} / {s2[3]} winners, V {s1[0].shape[0]} -> {g2[0].shape[0]}; flip round {g3[1]} / {s3[3]} winners")
    assert np.array_equal(got_target.view(np.int32), target.view(np.int32))
    for got, want in ((g1, s1), (g2, s2)):
        assert got[3] == want[3] and _same(got[1], want[1]) and _same(got[0], want[0]) and _same(got[2], want[2])
    assert g3[1] == s3[3] and _same(g3[0], s3[1])
    assert s1[3] > 0 and s2[3] > 0                                       # split and collapse have work on every case
    assert s3[3] > 0 or name != "uvsphere"                               # elsewhere the angle guard leaves no flip at this state
    assert torch.equal(before, _dev(s1[0])[0])                           # a round never writes its input
    # relax, on the mesh as given
    v, fc = rm.mesh(name)
    runs = [postprocess.remesh_relax(v.cuda(), fc.cuda(), RELAX) for _ in range(2)]
    x64 = rm.relax_restated(v.numpy(), fc.numpy(), RELAX, np.float64)
    e, unit = rc.rel_l2(runs[0], x64), float(gold[f"relax/{name}/ref_err"])
    fixed = torch.as_tensor(rm.tables(fc.numpy(), v.shape[0])["vflag"] != 0)
    print(f"relax {name}: rel-L2 vs float64 / unit {e:.2e}/{unit:.2e}={e / unit:.2f}; fixed vertices {int(fixed.sum())} of {v.shape[0]}, "
          f"moved {int((runs[0].cpu() != v).any(1).sum())}")
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0].cpu()[fixed], v[fixed])
    assert e <= MARGIN * unit


def test_the_known_flip_and_its_guards(hip_lib):
    from meshdiffusion_amd import postprocess
    v, f, even = rm.flip_patch()
    long, bent = v.copy(), v.copy()
    long[:, :2] = v[:, :2] + (v[:, :1] + v[:, 1:2])                       # stretched along (1, 1): the flip would lower the smallest angle
    bent[21, 2] = 2.0                                                    # the two faces meet at more than 30 degrees
    cos2 = float(rm.cos2_of(30.0))
    for tag, x, winners in (("flat", v, 1), ("stretched", long, 0), ("bent", bent, 0)):
        want, n = rm.flip_round_restated(x, f, cos2)
        got, m = postprocess.remesh_flip_round(*_dev(x, f), cos2)
        print(f"\n{tag}: winners {m} / {n}, slots rewritten {int((got.cpu() != torch.as_tensor(f)).any(1).sum())}")
        assert m == n == winners and _same(got, want)
    assert sorted(map(tuple, rm.flip_round_restated(v, f, cos2)[0].tolist())) != sorted(map(tuple, f.tolist()))


# ---- 2: the whole pipeline without relax is exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rm.PIPELINE_CASES)
def test_pipeline_without_relax_equals_the_restatement(hip_lib, name):
    x, f, vm, info = _run(name, 1.0, 0.0)
    wx, wf, wvm, winfo = rm.pipeline_restated(name, 1.0, 0.0)
    print(f"\n{name} relax 0 iters {rm.PIPELINE_ITERS}: V {x.shape[0]} / {wx.shape[0]} F {f.shape[0]} / {wf.shape[0]}; per iteration (splits, "
          f"collapses, flips, collapse rounds, flip rounds) {_rounds(info)} / {_rounds(winfo)}")
    assert _rounds(info) == _rounds(winfo) and np.array_equal(info["target"].view(np.int32), winfo["target"].view(np.int32))
    assert _same(f, wf) and _same(x, wx) and _same(vm, wvm)
    assert x.dtype == torch.float32 and f.dtype == torch.int64 and vm.dtype == torch.int32


# ---- 3: the whole pipeline with relax: conditions by construction ---------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", [(n, 1.0) for n in rm.CLOSED] + [("tetra", 10.0), ("octa", 10.0), ("uvsphere48", 1.0)])
def test_closed_meshes_stay_valid_manifolds(hip_lib, name, scale):
    v, f = rm.mesh(name)
    x, g, vm, info = _run(name, scale, RELAX, 3 if name == "uvsphere48" else rm.PIPELINE_ITERS)
    bad = rm.problems(g.cpu().numpy(), x.shape[0])
    chi = rm.euler(g.cpu().numpy(), vm.cpu().numpy(), 1)
    caps = [(r["collapse_rounds"] == rm.COLLAPSE_ROUNDS, r["flip_rounds"] == rm.FLIP_ROUNDS) for r in info["iterations"]]
    print(f"\n{name} x {scale}: V {v.shape[0]} -> {x.shape[0]} F {f.shape[0]} -> {g.shape[0]} chi {chi} per iteration {_rounds(info)} "
          f"round caps reached (collapse, flip) {caps} problems {bad[:4]}")
    assert bad == [] and chi == rm.euler(f.numpy(), np.zeros(v.shape[0], np.int64), 1) and g.shape[0] >= 4
    assert bool(torch.isfinite(x).all()) and int(vm.max()) == 0
    if name == "tetra":
        assert torch.equal(g.cpu(), f)


@pytest.mark.parametrize("name", ("fan40", "quad"))
def test_open_meshes_keep_their_boundary(hip_lib, name):
    v, f = rm.mesh(name)
    x, g, vm, info = _run(name)
    xn, gn = x.cpu().numpy(), g.cpu().numpy()
    key = lambda a: {r.tobytes() for r in np.ascontiguousarray(a)}
    b0, b1 = rm.boundary_vertices(f.numpy(), v.shape[0]), rm.boundary_vertices(gn, xn.shape[0])
    bad = rm.problems(gn, xn.shape[0], closed=False)
    print(f"\n{name}: V {v.shape[0]} -> {xn.shape[0]} F {f.shape[0]} -> {gn.shape[0]} boundary vertices {b0.shape[0]} -> {b1.shape[0]} per iteration "
          f"{_rounds(info)} problems {bad[:4]}")
    assert bad == [] and rm.euler(gn, vm.cpu().numpy(), 1) == [1]
    assert key(v.numpy()[b0]) <= key(xn[b1])                             # every original boundary vertex is still there, bit for bit


def test_degenerate_input_returns(hip_lib):
    v, f = rm.mesh("degen")
    x, g, vm, info = _run("degen")
    gn = g.cpu().numpy()
    proper = gn[~rm.repeated(gn)]
    bad = [p for p in rm.problems(proper, x.shape[0], closed=False) if "unreferenced" not in p]
    print(f"\ndegen: V {v.shape[0]} -> {x.shape[0]} F {f.shape[0]} -> {gn.shape[0]} per iteration {_rounds(info)} problems of the proper faces {bad}")
    assert gn.min() >= 0 and gn.max() < x.shape[0] and bool(torch.isfinite(x).all()) and bad == []
    wx, wf, _, _ = rm.pipeline_restated("degen", 1.0, 0.0)
    x0, g0, _, _ = _run("degen", 1.0, 0.0)
    assert _same(g0, wf) and _same(x0, wx)


@pytest.mark.parametrize("name,scale", rm.QUALITY_CASES)
def test_quality_improves(hip_lib, gold, name, scale):
    v, f = rm.mesh(name)
    x, g, vm, info = _run(name, scale)
    L = float(info["target"][0])
    before, after = rm.quality(v.numpy(), f.numpy(), L), rm.quality(x.cpu().numpy(), g.cpu().numpy(), L)
    key = f"quality/{name}/{scale}"
    wx, wf, _, _ = rm.pipeline_restated(name, scale, RELAX)
    print(f"\n{name} x {scale}: L {L:.4f} F {f.shape[0]} -> {g.shape[0]} (restatement {int(gold[key + '/faces_after'])}); band share "
          f"{before[0]:.3f} -> {after[0]:.3f} (restatement {float(gold[key + '/share_after']):.3f}); minimum angle {before[1]:.1f} -> "
          f"{after[1]:.1f} (restatement {float(gold[key + '/angle_after']):.1f}); faces equal the restatement's: {_same(g, wf)}; "
          f"max |x - restatement| {float((x.cpu() - torch.as_tensor(wx)).abs().max()) if x.shape[0] == wx.shape[0] else float('nan'):.2e}")
    assert rm.problems(g.cpu().numpy(), x.shape[0]) == []
    assert after[0] > before[0]
    assert after[1] > before[1]


def test_fidelity_on_the_unit_sphere(hip_lib, gold):
    from meshdiffusion_amd import pointcloud
    v, f = rm.mesh("uvsphere")
    x, g, vm, info = _run("uvsphere")
    dev, unit = float((x.double().norm(dim=1) - 1).abs().max()), float(gold["fidelity/uvsphere/radial_dev"])
    uni = torch.rand(3, 1, 2048, generator=torch.Generator().manual_seed(11)).cuda()
    p0 = pointcloud.sample_points(v.cuda()[None], f.cuda(), 2048, uniforms=uni)[0]
    p1 = pointcloud.sample_points(x[None], g, 2048, uniforms=uni)[0]
    cd = float(pointcloud.chamfer_distance(p0, p1)[0])
    print(f"\nuvsphere: max | |x| - 1 | {dev:.4f} (restatement {unit:.4f}); symmetric squared chamfer distance of 2048 samples {cd:.3e}")
    assert dev <= 2 * unit


# ---- 4: batch and repeatability -----------------------------------------------------------------------------------------------------
def test_batch_equals_its_halves_and_two_runs_agree(hip_lib):
    from meshdiffusion_amd import postprocess
    both, a, b = _run("pair"), _run("ptorus"), _run("fan40")
    print(f"\npair: V {both[0].shape[0]} = {a[0].shape[0]} + {b[0].shape[0]}, F {both[1].shape[0]} = {a[1].shape[0]} + {b[1].shape[0]}")
    assert torch.equal(both[0], torch.cat([a[0], b[0]])) and torch.equal(both[1], torch.cat([a[1], b[1] + a[0].shape[0]]))
    assert torch.equal(both[2], torch.cat([a[2], b[2] + 1])) and _rounds(both[3])[0][0] == _rounds(a[3])[0][0] + _rounds(b[3])[0][0]
    v, f = rm.mesh("pair")
    dv, df, dvm = v.cuda(), f.cuda(), rm.vert_mesh("pair").cuda()
    keep = (dv.clone(), df.clone(), dvm.clone())
    again = postprocess.remesh(dv, df, iters=rm.PIPELINE_ITERS, vert_mesh=dvm)
    assert all(torch.equal(p, q) for p, q in zip(again[:3], both[:3])) and _rounds(again[3]) == _rounds(both[3])
    assert torch.equal(dv, keep[0]) and torch.equal(df, keep[1]) and torch.equal(dvm, keep[2])        # the input is never written
    # per-mesh targets: each half alone at its own length
    t = both[3]["target"]
    own = postprocess.remesh(dv, df, iters=2, target_len=torch.as_tensor(t), vert_mesh=dvm)
    auto = postprocess.remesh(dv, df, iters=2, vert_mesh=dvm)
    assert torch.equal(own[0], auto[0]) and torch.equal(own[1], auto[1])
    halves = [(rm.mesh(n)[0].cuda(), rm.mesh(n)[1].cuda()) for n in ("ptorus", "fan40")]
    today = postprocess.postprocess(halves, smooth_steps=2, keep_largest=True)
    same = postprocess.postprocess(halves, smooth_steps=2, keep_largest=True, remesh_iters=0, remesh_target_scale=0.7)
    assert all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(today, same))      # remesh_iters = 0: today's tensors
    out = postprocess.postprocess(halves, smooth_steps=2, remesh_iters=2)
    x, g, vm, _ = postprocess.remesh(dv, df, iters=2, vert_mesh=dvm)
    x = postprocess.smooth(x, g, 2)
    x, g, vm, _ = postprocess.remesh(x, g, iters=2, vert_mesh=vm)
    want = postprocess.split_meshes(x, g, vm, 2)
    assert all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(out, want))        # remesh, smooth, remesh


# ---- 5: the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_remeshes(hip_lib, tmp_path):
    from meshdiffusion_amd import mesh_export
    samples = mc.sphere_and_blob_samples(M=1)
    np.save(tmp_path / "samples.npy", samples)
    tet = os.path.join(GOLD, "64_tets_cropped.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "meshdiffusion_amd.mesh_export", "--sample_path", str(tmp_path / "samples.npy"), "--tet_path", tet,
                        "--out", str(tmp_path / "remeshed"), "--remesh_iters", "2", "--num_smooth_steps", "2", "--preview_dir",
                        str(tmp_path / "png"), "--preview_post", "--preview_res", "128"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout[-500:], r.stderr[-2000:])
    assert r.returncode == 0
    t = np.load(tet)
    plain = mesh_export.samples_to_obj(samples, t["vertices"], t["indices"], str(tmp_path / "plain"))
    named = mesh_export.samples_to_obj(samples, t["vertices"], t["indices"], str(tmp_path / "named"), remesh_iters=0, remesh_target_scale=1.0)
    assert open(plain[0], "rb").read() == open(named[0], "rb").read()    # the new keywords at their defaults: the same bytes
    v0, f0 = mesh_export.load_obj(plain[0])
    v1, f1 = mesh_export.load_obj(str(tmp_path / "remeshed" / "000000.obj"))
    L = float(rm.default_target(v0, f0, np.zeros(v0.shape[0], np.int64), 1)[0])
    q0, q1 = rm.quality(v0, f0, L), rm.quality(v1, f1, L)
    bad = rm.problems(f1, v1.shape[0])
    img = mesh_export.load_png(str(tmp_path / "png" / "000000.png"))
    print(f"marching tetrahedra V {v0.shape[0]} F {f0.shape[0]} share {q0[0]:.3f} min angle {q0[1]:.1f} -> V {v1.shape[0]} F {f1.shape[0]} share "
          f"{q1[0]:.3f} min angle {q1[1]:.1f}; components {len(np.unique(mc.components_restated(f1, v1.shape[0])[0]))}; problems {bad[:4]}")
    assert rm.problems(f0, v0.shape[0]) == [] and bad == [] and np.isfinite(v1).all()
    assert len(np.unique(mc.components_restated(f1, v1.shape[0])[0])) == 2 and img.shape == (128, 128, 3) and int((img != 255).any(-1).sum()) > 100
