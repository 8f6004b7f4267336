"""The mesh distance on the GPU (csrc/meshdist.hip, meshdiffusion_amd/meshdist.py, postprocess.remesh(project=True),
python -m meshdiffusion_amd.mesh_export --remesh_project) against the restatements of tests/meshdist_cases.py.

Bars, none fitted to what the kernel gives:
  closest point     dist2, face and closest torch.equal with the float32 restatement (the bar tests/test_gpu_remesh.py holds the
                    remesher to), and rel-L2 against the float64 restatement <= 4 x the float32 restatement's OWN rel-L2 distance
                    from float64 for that case and query set, recorded in tests/golden/meshdist.npz by tools/gen_golden_meshdist.py
                    (the margin of tests/test_gpu_meshpost.py and tests/test_gpu_fixedtopo.py).
  winding number    max-abs against float64 <= 4 x the float32 restatement's own max-abs distance from float64 (the same file); on the
                    closed cases |w| >= 0.5 as in float64 for every lattice query; two runs and the one- and all-output launches
                    bit-equal.
  warm start        every extracted vertex within the longest tet edge of the target: the vertex lies on a grid edge whose ends have
                    opposite signs of a field that changes sign only across the closed target, so the target crosses that edge.
  re-projection     torch.equal with remesh_with_projection_restated; every output vertex's float64 distance to the input surface <=
                    4 x (the case's lattice unit of `closest`, a relative figure) x (the largest norm of an input vertex, the scale
                    of the coordinates the closest point is rounded at).
Each test prints its figures before it asserts.
"""
import functools
import os

import numpy as np
import pytest
import torch

import meshdist_cases as md
import meshpost_cases as mc
import remesh_cases as rm
from conftest import GOLD

pytestmark = pytest.mark.gpu
MARGIN = 4.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "meshdist.npz"))


@functools.lru_cache(maxsize=None)
def _gpu_case(name):
    v, f = rm.mesh(name)
    return v.cuda(), f.cuda(), rm.vert_mesh(name).cuda()


@functools.lru_cache(maxsize=None)
def _gpu_queries(name, which):
    p, pm = md.queries(name, which)
    return torch.from_numpy(p).cuda(), torch.from_numpy(pm).cuda()


def _same(got, want):
    """bit-equality of float tensors, NaN == NaN included."""
    got, want = torch.as_tensor(got).cpu(), torch.as_tensor(want).cpu()
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                                                                               want.view(torch.int32) if want.dtype == torch.float32 else want)


def _check_closest(got, want, tag):
    d2, face, close = (t.cpu() for t in got)
    wd2, wface, wclose = (torch.from_numpy(a) for a in want)
    print(f"\n{tag}: Q {d2.shape[0]} dist2 differs at {int((d2 != wd2).sum())}, face at {int((face != wface).sum())}, "
          f"closest at {int((close != wclose).any(1).sum())} queries")
    assert face.dtype == torch.int64 and torch.equal(face, wface), tag
    assert torch.equal(d2, wd2) and torch.equal(close, wclose), tag


# ---- closest point ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", md.QUERY_SETS)
@pytest.mark.parametrize("name", md.CASES)
def test_closest_point_equals_the_restatement_and_float64(hip_lib, gold, name, which):
    from meshdiffusion_amd import meshdist
    v, f, vm = _gpu_case(name)
    p, pm = _gpu_queries(name, which)
    p0 = p.clone()
    got = meshdist.closest_point(p, v, f, point_mesh=pm, vert_mesh=vm)
    _check_closest(got, md.case_closest(name, which, np.float32), f"{name} {which}")
    d64, _, c64 = md.case_closest(name, which, np.float64)
    ec, ed = md.rel_l2(got[2].cpu().numpy(), c64), md.rel_l2(np.sqrt(got[0].cpu().numpy().astype(np.float64)), np.sqrt(d64))
    uc, ud = float(gold[f"closest/{name}/{which}/unit_closest"]), float(gold[f"closest/{name}/{which}/unit_dist"])
    print(f"against float64: closest {ec:.2e} (unit {uc:.2e}), sqrt(dist2) {ed:.2e} (unit {ud:.2e})")
    assert ec <= MARGIN * uc and ed <= MARGIN * ud
    assert torch.equal(p, p0)                                            # the inputs are never written


@pytest.mark.parametrize("T", (1, md.TILE - 1, md.TILE, md.TILE + 1, 9024))
def test_closest_point_at_the_tile_and_block_edges(hip_lib, gold, T):
    from meshdiffusion_amd import meshdist
    v, f, _ = _gpu_case(md.BIG)
    tri = md.case_triangles(md.BIG)[0]
    want = md.case_closest(md.BIG, "lattice", np.float32) if T == 9024 else md.closest_restated(md.lattice(), tri[:T])
    p = torch.from_numpy(md.lattice()).cuda()
    for Q in (1, 255, 256, 257, 729):
        got = meshdist.closest_point(p[:Q], v, f[:T])
        _check_closest(got, tuple(a[:Q] for a in want), f"T {T} Q {Q}")
    if T == 9024:
        d64, _, c64 = md.case_closest(md.BIG, "lattice", np.float64)
        ec, ed = md.rel_l2(got[2].cpu().numpy(), c64), md.rel_l2(np.sqrt(got[0].cpu().numpy().astype(np.float64)), np.sqrt(d64))
        uc, ud = float(gold[f"closest/{md.BIG}/lattice/unit_closest"]), float(gold[f"closest/{md.BIG}/lattice/unit_dist"])
        print(f"against float64: closest {ec:.2e} (unit {uc:.2e}), sqrt(dist2) {ed:.2e} (unit {ud:.2e})")
        assert ec <= MARGIN * uc and ed <= MARGIN * ud


# ---- winding number --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", md.CASES + (md.BIG,))
def test_winding_number_against_float64(hip_lib, gold, name):
    from meshdiffusion_amd import meshdist
    v, f, vm = _gpu_case(name)
    p, pm = _gpu_queries(name, "lattice")
    w = meshdist.winding_number(p, v, f, point_mesh=pm, vert_mesh=vm)
    again = meshdist.winding_number(p, v, f, point_mesh=pm, vert_mesh=vm)
    w64 = md.case_winding(name, np.float64)
    err, unit = md.max_abs(w.cpu().numpy(), w64), float(gold[f"winding/{name}/unit"])
    print(f"\n{name}: Q {w.shape[0]} max-abs against float64 {err:.2e} (unit {unit:.2e}), against the float32 restatement "
          f"{md.max_abs(w.cpu().numpy(), md.case_winding(name, np.float32)):.2e}")
    assert w.dtype == torch.float32 and bool(torch.isfinite(w).all()) and _same(w, again)
    assert err <= MARGIN * unit
    if name in md.CLOSED or name == md.BIG:
        inside = np.abs(w64) >= 0.5
        assert np.array_equal(w.abs().cpu().numpy() >= 0.5, inside) and 0 < inside.sum() < inside.shape[0]


@pytest.mark.parametrize("name", ("ptorus", "pair", "degen"))
def test_one_launch_for_all_outputs_equals_the_single_launches(hip_lib, name):
    from meshdiffusion_amd import meshdist
    v, f, vm = _gpu_case(name)
    p, pm = _gpu_queries(name, "lattice")
    tri, tri_ptr, face_of, M = meshdist.mesh_triangles(v, f, vm)
    both = meshdist.mesh_query(p, tri, tri_ptr, face_of, M, pm, "test", True, True)
    close = meshdist.closest_point(p, v, f, point_mesh=pm, vert_mesh=vm)
    wind = meshdist.winding_number(p, v, f, point_mesh=pm, vert_mesh=vm)
    assert all(_same(a, b) for a, b in zip(both[:3], close)) and _same(both[3], wind)
    sdf, face, closest = meshdist.signed_distance(p, v, f, point_mesh=pm, vert_mesh=vm)
    want = torch.sqrt(close[0].double()).float() * torch.where(wind.abs() >= 0.5, 1.0, -1.0)
    print(f"\n{name}: {int((sdf > 0).sum())} of {sdf.shape[0]} queries inside")
    assert _same(sdf, want) and _same(face, close[1]) and _same(closest, close[2])
    if name == "ptorus":                                                 # wound inward: w = -1 inside, the field is positive there all the same
        assert bool((wind[sdf > 0] < -0.5).all()) and int((sdf > 0).sum()) == int((np.abs(md.case_winding(name, np.float64)) >= 0.5).sum())


# ---- batches -----------------------------------------------------------------------------------------------------------------------
def test_a_batch_equals_its_meshes_and_an_empty_mesh_takes_nothing(hip_lib):
    from meshdiffusion_amd import meshdist
    v, f, vm = _gpu_case("pair")
    p, pm = _gpu_queries("pair", "lattice")
    both = meshdist.mesh_query(p, *meshdist.mesh_triangles(v, f, vm), pm, "test", True, True)
    F0 = rm.mesh("ptorus")[1].shape[0]
    for m, name in enumerate(("ptorus", "fan40")):
        hv, hf, _ = _gpu_case(name)
        one = meshdist.mesh_query(p[pm == m], *meshdist.mesh_triangles(hv, hf), None, "test", True, True)
        sel = (pm == m).cpu()
        assert _same(both[0].cpu()[sel], one[0]) and _same(both[2].cpu()[sel], one[2]) and _same(both[3].cpu()[sel], one[3]), name
        assert torch.equal(both[1].cpu()[sel], one[1].cpu() + m * F0), name
    # octa, three loose vertices without a face, tetra
    parts = [rm.mesh("octa"), (torch.eye(3), torch.zeros(0, 3, dtype=torch.int64)), rm.mesh("tetra")]
    cv, cf, cvm = mc.concat(parts)
    lat = torch.from_numpy(md.lattice()).cuda()
    q, qm = torch.cat([lat[:300], lat[:257], lat]), torch.cat([torch.full((n,), m) for m, n in enumerate((300, 257, 729))]).cuda()
    d2, face, close, wind = meshdist.mesh_query(q, *meshdist.mesh_triangles(cv.cuda(), cf.cuda(), cvm.cuda()), qm, "test", True, True)
    for m, (n, base) in enumerate(((300, 0), (257, 0), (729, 8))):
        sel = (qm == m).cpu()
        if m == 1:
            print(f"\nthe empty mesh: dist2 {d2.cpu()[sel][:3].tolist()} face {face.cpu()[sel][:3].tolist()} winding {wind.cpu()[sel][:3].tolist()}")
            assert bool(torch.isinf(d2.cpu()[sel]).all()) and bool((d2.cpu()[sel] > 0).all()) and bool((face.cpu()[sel] == -1).all())
            assert _same(close.cpu()[sel], lat[:n]) and bool((wind.cpu()[sel] == 0).all())
            continue
        hv, hf = parts[m]
        one = meshdist.mesh_query(lat[:n], *meshdist.mesh_triangles(hv.cuda(), hf.cuda()), None, "test", True, True)
        assert _same(d2.cpu()[sel], one[0]) and _same(close.cpu()[sel], one[2]) and _same(wind.cpu()[sel], one[3]), m
        assert torch.equal(face.cpu()[sel], one[1].cpu() + base), m


def test_ungrouped_faces_give_the_same_answer_with_indices_mapped_back(hip_lib):
    from meshdiffusion_amd import meshdist
    v, f, vm = _gpu_case("pair")
    F0, F = rm.mesh("ptorus")[1].shape[0], f.shape[0]
    # the faces of the second mesh dealt in among those of the first, each mesh keeping its own order: the stable sort by mesh
    # restores the grouped list, so the answers are the grouped ones and only the face numbers change
    key = np.concatenate([np.arange(F0, dtype=np.float64), (np.arange(F - F0) * (F0 / (F - F0))) - 0.5])
    perm = torch.from_numpy(np.argsort(key, kind="stable")).cuda()
    fm = vm.long()[f[perm][:, 0]]
    assert bool((fm[1:] < fm[:-1]).any())                                # not grouped
    for which in md.QUERY_SETS:
        p, pm = _gpu_queries("pair", which)
        want = meshdist.closest_point(p, v, f, point_mesh=pm, vert_mesh=vm)
        got = meshdist.closest_point(p, v, f[perm], point_mesh=pm, vert_mesh=vm)
        print(f"\npair {which}, faces dealt in: the face numbers differ at {int((got[1] != want[1]).sum())} of {p.shape[0]} queries before mapping")
        assert _same(got[0], want[0]) and _same(got[2], want[2]) and torch.equal(perm[got[1]], want[1])
        assert torch.equal(fm[got[1]], pm.long())                        # the mesh of a face is that of its first vertex
        assert _same(meshdist.winding_number(p, v, f[perm], point_mesh=pm, vert_mesh=vm), meshdist.winding_number(p, v, f, point_mesh=pm, vert_mesh=vm))


# ---- non-finite values -----------------------------------------------------------------------------------------------------------
def test_nan_queries_nan_corners_and_degenerate_faces_follow_the_contract(hip_lib, gold):
    from meshdiffusion_amd import meshdist
    v, f, _ = _gpu_case("octa")
    tri = md.case_triangles("octa")[0]
    p = md.lattice().copy()
    p[[5, 300, 728]] = [(np.nan, 0, 0), (0.1, np.nan, 0.2), (np.inf, 0, 0)]
    got = meshdist.closest_point(torch.from_numpy(p).cuda(), v, f)
    want = md.closest_restated(p, tri)
    clean = md.case_closest("octa", "lattice", np.float32)
    print(f"\nNaN / inf queries: dist2 {got[0][[5, 300, 728]].tolist()} face {got[1][[5, 300, 728]].tolist()}")
    assert all(_same(a, torch.from_numpy(b)) for a, b in zip(got, want))
    assert got[1][[5, 300, 728]].tolist() == [-1, -1, -1] and bool(torch.isinf(got[0][[5, 300, 728]]).all())
    keep = np.setdiff1d(np.arange(729), [5, 300, 728])
    assert all(_same(a.cpu()[keep], torch.from_numpy(b[keep])) for a, b in zip(got, clean))        # the other queries are untouched
    w = meshdist.winding_number(torch.from_numpy(p).cuda(), v, f).cpu().numpy()
    w64 = md.winding_restated(p, tri, dtype=np.float64)
    print(f"winding at the three: {w[[5, 300, 728]].tolist()}; float64 {w64[[5, 300, 728]].tolist()}")
    assert np.array_equal(np.isnan(w), np.isnan(w64)) and np.isnan(w[[5, 300]]).all()
    assert md.max_abs(w[keep], w64[keep]) <= MARGIN * float(gold["winding/octa/unit"])
    # a NaN corner: that triangle is never taken, the winding number of its mesh is NaN
    vb = v.clone()
    vb[4, 1] = float("nan")                                              # vertex 4 is a corner of faces 0..3
    tb = vb.cpu().numpy()[f.cpu().numpy()]
    got = meshdist.closest_point(torch.from_numpy(md.lattice()).cuda(), vb, f)
    want = md.closest_restated(md.lattice(), tb)
    print(f"a NaN corner: faces taken {sorted(set(got[1].tolist()))}")
    assert all(_same(a, torch.from_numpy(b)) for a, b in zip(got, want)) and int(got[1].min()) >= 4
    assert bool(torch.isnan(meshdist.winding_number(torch.from_numpy(md.lattice()).cuda(), vb, f)).all())
    # the degenerate mesh: both query sets equal the restatement in test_closest_point_equals_the_restatement_and_float64; here the
    # pattern of what is finite
    dv, df, _ = _gpu_case("degen")
    got = meshdist.closest_point(_gpu_queries("degen", "lattice")[0], dv, df)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all()) and bool((got[1] >= 0).all())


# ---- the warm start of the fit -------------------------------------------------------------------------------------------------------
def test_warm_start_extracts_the_target_within_one_tet_edge(hip_lib):
    from meshdiffusion_amd import meshdist
    from meshdiffusion_amd.dmtet import DMTetGeometry
    tet = np.load(os.path.join(GOLD, "64_tets_cropped.npz"))
    torch.manual_seed(0)
    geo = DMTetGeometry(64, 2.1, None, tets=(tet["vertices"], tet["indices"]), deform_scale=2.0)
    v, f = rm.mesh("uvsphere")
    tv = (v * 0.8).cuda()
    before = geo.sdf.detach().clone()
    sdf = meshdist.init_sdf(geo, tv, f.cuda())
    assert _same(geo.sdf.detach(), sdf) and not torch.equal(before, sdf) and float(sdf.abs().max()) <= 1.0
    with torch.no_grad():
        mesh = geo.getMesh()
    x = mesh.v_pos.detach().cpu().numpy()
    tri = (v * 0.8).numpy()[f.numpy()]
    dist = np.sqrt(md.closest_restated(x, tri, dtype=np.float64)[0])
    e = geo.verts[geo.all_edges.reshape(-1, 2)].double()
    longest = float((e[:, 0] - e[:, 1]).norm(dim=1).max())
    print(f"\nwarm start: grid vertices {geo.verts.shape[0]} inside {int((sdf > 0).sum())}; extracted V {x.shape[0]} F {mesh.t_pos_idx.shape[0]}; "
          f"distance to the target mean {dist.mean():.4f} max {dist.max():.4f}; longest tet edge {longest:.4f}")
    assert x.shape[0] > 0 and mesh.t_pos_idx.shape[0] > 0
    assert dist.max() <= longest
    idx = np.random.default_rng(7).choice(geo.verts.shape[0], 2000, replace=False)
    q = geo.verts[idx].cpu().numpy()
    d2 = md.closest_restated(q, tri)[0]
    w64 = md.winding_restated(q, tri, dtype=np.float64)
    assert np.abs(np.abs(w64) - 0.5).min() > 0.4                         # no sampled grid vertex sits on the target
    want = np.clip(np.where(np.abs(w64) >= 0.5, 1, -1).astype(np.float32) * np.sqrt(d2), -1, 1)
    assert _same(sdf.cpu()[idx], torch.from_numpy(want))


# ---- the re-projection of the remesher -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", md.PROJECT_CASES)
def test_remesh_with_projection_equals_the_restatement(hip_lib, gold, name):
    from meshdiffusion_amd import postprocess
    v, f, vm = _gpu_case(name)
    v0, f0 = v.clone(), f.clone()
    kw = dict(iters=md.PROJECT_ITERS, relax=0.5, vert_mesh=vm)
    x, g, gm, info = postprocess.remesh(v, f, project=True, **kw)
    x2, g2, gm2, info2 = postprocess.remesh(v, f, project=True, **kw)
    wx, wg, wm, winfo = md.project_restated(name, True)
    print(f"\n{name}: V {v.shape[0]} -> {x.shape[0]} F {f.shape[0]} -> {g.shape[0]}; per iteration {[tuple(r.values()) for r in info['iterations']]}; "
          f"restated {[tuple(r.values()) for r in winfo['iterations']]}")
    assert torch.equal(g.cpu(), torch.from_numpy(wg)) and torch.equal(gm.cpu(), torch.from_numpy(wm)) and _same(x, torch.from_numpy(wx))
    assert info["iterations"] == winfo["iterations"] and all("max_project_dist2" in r for r in info["iterations"])
    assert _same(x, x2) and torch.equal(g, g2) and torch.equal(gm, gm2) and info2["iterations"] == info["iterations"]
    assert torch.equal(v, v0) and torch.equal(f, f0)
    # without the flag: today's remesh, bit for bit
    px, pg, pm_, pinfo = postprocess.remesh(v, f, **kw)
    tx, tg, tm, tinfo = rm.remesh_restated(rm.mesh(name)[0].numpy(), rm.mesh(name)[1].numpy(), iters=md.PROJECT_ITERS, relax=0.5,
                                           vert_mesh=rm.vert_mesh(name).numpy())
    assert _same(px, torch.from_numpy(tx)) and torch.equal(pg.cpu(), torch.from_numpy(tg)) and torch.equal(pm_.cpu(), torch.from_numpy(tm))
    assert pinfo["iterations"] == tinfo["iterations"] and not any("max_project_dist2" in r for r in pinfo["iterations"])
    # fidelity and quality, next to the recorded figures of the restated pipeline
    dist = md.surface_distance64((x.cpu().numpy(), gm.cpu().numpy()), name)
    unit = float(gold[f"closest/{name}/lattice/unit_closest"])
    scale = float(np.linalg.norm(rm.mesh(name)[0].numpy().astype(np.float64), axis=1).max())
    for tag, (mx, mf, mm, mi) in (("on", (x, g, gm, info)), ("off", (px, pg, pm_, pinfo))):
        fig = md.project_figures(name, mx.cpu().numpy(), mf.cpu().numpy(), mm.cpu().numpy(), mi["target"])
        rec = tuple(float(gold[f"project/{name}/{tag}/{k}"]) for k in ("share", "angle", "mean_dist", "max_dist"))
        print(f"project {tag}: share {fig[0]:.3f} min angle {fig[1]:.1f} distance mean {fig[2]:.2e} max {fig[3]:.2e}; recorded "
              f"{rec[0]:.3f} {rec[1]:.1f} {rec[2]:.2e} {rec[3]:.2e}")
        assert fig == rec and mf.shape[0] == int(gold[f"project/{name}/{tag}/faces"])
    print(f"distance of the projected vertices to the input surface: max {dist.max():.2e}; bar {MARGIN} x {unit:.2e} x {scale:.3f} = "
          f"{MARGIN * unit * scale:.2e}")
    assert dist.max() <= MARGIN * unit * scale


def test_remesh_with_projection_of_a_batch_equals_its_halves(hip_lib):
    from meshdiffusion_amd import postprocess
    v, f, vm = _gpu_case("pair")
    kw = dict(iters=md.PROJECT_ITERS, relax=0.5, project=True)
    x, g, gm, info = postprocess.remesh(v, f, vert_mesh=vm, **kw)
    halves = [postprocess.remesh(*_gpu_case(n)[:2], **kw) for n in ("ptorus", "fan40")]
    assert _same(x, torch.cat([h[0] for h in halves])) and torch.equal(g, torch.cat([halves[0][1], halves[1][1] + halves[0][0].shape[0]]))
    assert torch.equal(gm.cpu(), torch.cat([torch.full((h[0].shape[0],), k, dtype=torch.int32) for k, h in enumerate(halves)]))
    for k, rec in enumerate(info["iterations"]):
        assert rec["max_project_dist2"] == max(h[3]["iterations"][k]["max_project_dist2"] for h in halves)


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_command_line_without_the_flag_is_unchanged_and_with_it_projects(hip_lib, tmp_path):
    from meshdiffusion_amd import mesh_export
    samples = mc.sphere_and_blob_samples()
    np.save(tmp_path / "samples.npy", samples)
    tet = os.path.join(GOLD, "64_tets_cropped.npz")
    base = ["--sample_path", str(tmp_path / "samples.npy"), "--tet_path", tet]
    mesh_export.main(base + ["--out", str(tmp_path / "plain")])
    mesh_export.main(base + ["--out", str(tmp_path / "remesh"), "--remesh_iters", "1", "--keep_largest"])
    mesh_export.main(base + ["--out", str(tmp_path / "project"), "--remesh_iters", "1", "--keep_largest", "--remesh_project"])
    t = np.load(tet)
    api = mesh_export.samples_to_obj(samples, t["vertices"], t["indices"], str(tmp_path / "api"))
    api_remesh = mesh_export.samples_to_obj(samples, t["vertices"], t["indices"], str(tmp_path / "api_remesh"), remesh_iters=1, keep_largest=True)
    for k, path in enumerate(api):
        name = os.path.basename(path)
        assert open(path, "rb").read() == open(tmp_path / "plain" / name, "rb").read()
        assert open(api_remesh[k], "rb").read() == open(tmp_path / "remesh" / name, "rb").read()
        v0, f0 = mesh_export.load_obj(str(tmp_path / "remesh" / name))
        v1, f1 = mesh_export.load_obj(str(tmp_path / "project" / name))
        raw_v, raw_f = mesh_export.load_obj(path)
        print(f"\nmesh {k}: raw {raw_v.shape[0]} / {raw_f.shape[0]}; remeshed {v0.shape[0]} / {f0.shape[0]}; with projection {v1.shape[0]} / {f1.shape[0]}")
        assert f1.shape[0] > 0 and int(f1.min()) >= 0 and int(f1.max()) < v1.shape[0] and np.isfinite(v1).all()
        assert not rm.repeated(np.asarray(f1)).any()
        assert open(tmp_path / "project" / name, "rb").read() != open(tmp_path / "remesh" / name, "rb").read()
