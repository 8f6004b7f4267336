"""Host side of the mesh distance (csrc/meshdist.hip, meshdiffusion_amd/meshdist.py) without a GPU: the export's tables, its
refusals in their stated order through the loaded library (nothing is launched), the Python wrappers' refusals, the numpy restatement
of tests/meshdist_cases.py against hand-made answers and against float64, and the recorded figures.  Each test prints its figures
before it asserts."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import meshdist_cases as md
import remesh_cases as rm
from conftest import GOLD, ROOT


def test_the_export_is_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import _lib, build, meshdist, postprocess
    header = open(os.path.join(ROOT, "include", "meshdiffusion_hip.h")).read()
    name = "md_mesh_query"
    n_args = len(re.search(rf"\bint {name}\(([^;]*)\);", header).group(1).split(","))
    print(f"\n{name}: {n_args} arguments in the header, {len(_lib.SIGNATURES[name][1])} in _lib.SIGNATURES")
    assert n_args == len(_lib.SIGNATURES[name][1]) == 12
    assert "meshdist.hip" in build.SOURCES
    assert _lib.MESHDIST_MAX_MESHES == 65535
    src = open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "meshdist.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "THE MESH DISTANCE CONTRACT" in src and "atomic" not in src.split("#include")[1]
    assert int(re.search(r"MDQ_THREADS = (\d+)", src).group(1)) == md.TILE and "MDQ_TILE = MDQ_THREADS" in src
    for fn in ("closest_point", "winding_number", "signed_distance", "init_sdf", "mesh_triangles"):
        assert callable(getattr(meshdist, fn)), fn
    assert "project" in postprocess.remesh.__kwdefaults__ and postprocess.remesh.__kwdefaults__["project"] is False
    assert postprocess.postprocess.__kwdefaults__["remesh_project"] is False


def test_the_export_refuses_in_its_stated_order_without_a_gpu(hip_lib):
    fn = hip_lib.md_mesh_query
    nul, odd = C.c_void_p(0), C.c_void_p(66)
    p = [C.c_void_p(64 * (k + 1)) for k in range(8)]                     # distinct, aligned, never dereferenced: nothing is launched
    BAD, UNSUPPORTED = -1, -2
    # md_mesh_query(tri, tri_ptr, query, query_ptr, T, Q, M, dist2, face, closest, winding, stream)
    ok = [p[0], p[1], p[2], p[3], 100, 100, 2, p[4], p[5], p[6], p[7], nul]
    big = 1 << 40

    def with_(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    # 1 pointers: required ones null or misaligned, optional ones misaligned, no output at all
    for k in (1, 2, 3):
        assert with_(**{f"a{k}": nul}) == BAD and with_(**{f"a{k}": odd}) == BAD, k
    for k in (0, 7, 8, 9, 10):
        assert with_(**{f"a{k}": odd}) == BAD, k
    assert with_(a7=nul, a8=nul, a9=nul, a10=nul) == BAD
    assert with_(a0=nul) == BAD                                          # no triangles to read, but T > 0
    # 2 counts
    for k in (4, 5, 6):
        assert with_(**{f"a{k}": -3}) == BAD, k
    # 3 limits
    assert with_(a4=big) == UNSUPPORTED and with_(a5=big) == UNSUPPORTED and with_(a4=1 << 31) == UNSUPPORTED
    assert with_(a6=65536) == UNSUPPORTED
    # 4 aliasing: an output that is an input
    for o in (7, 8, 9, 10):
        for i in (0, 1, 2, 3):
            assert with_(**{f"a{o}": ok[i]}) == BAD, (o, i)
    # the order: a pointer error hides a limit, a negative count hides a limit, a limit hides an alias
    assert with_(a1=nul, a4=big) == BAD and with_(a4=-1, a5=big) == BAD and with_(a4=big, a7=ok[0]) == UNSUPPORTED
    assert with_(a6=65536, a7=ok[2]) == UNSUPPORTED and with_(a5=0, a7=ok[2]) == BAD      # the alias is refused before Q == 0 returns
    # nothing to do: MD_OK without a launch (there is no GPU here, and every pointer is a made-up address)
    assert with_(a5=0) == 0 and with_(a6=0) == 0 and with_(a0=nul, a4=0, a5=0) == 0
    for keep in (7, 8, 9, 10):                                           # one output is enough
        a = {f"a{k}": nul for k in (7, 8, 9, 10) if k != keep}
        assert with_(a5=0, **a) == 0, keep


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from meshdiffusion_amd import _lib, meshdist, postprocess
    v, f = rm.mesh("octa")
    pts = torch.from_numpy(md.lattice())
    for fn in (meshdist.closest_point, meshdist.winding_number, meshdist.signed_distance):
        with pytest.raises(_lib.MeshDiffusionHipError):
            fn(pts, v, f)                                                # CPU tensors: no fallback
    with pytest.raises(_lib.MeshDiffusionHipError):
        postprocess.remesh(v, f, project=True)
    if torch.cuda.is_available():
        v, f, pts = v.cuda(), f.cuda(), pts.cuda()
        bad_calls = [lambda: meshdist.closest_point(pts[:, :2], v, f), lambda: meshdist.closest_point(pts, v[:, :2], f),
                     lambda: meshdist.closest_point(pts, v, f[:, :2]), lambda: meshdist.closest_point(pts, v, f + 1),
                     lambda: meshdist.closest_point(pts.long(), v, f), lambda: meshdist.closest_point(pts, v.long(), f),
                     lambda: meshdist.closest_point(pts[:3], v, f, point_mesh=torch.tensor([0, 1, 0])),
                     lambda: meshdist.closest_point(pts[:3], v, f, point_mesh=torch.tensor([0, 0, 1])),
                     lambda: meshdist.closest_point(pts[:3], v, f, point_mesh=torch.tensor([0, 0])),
                     lambda: meshdist.closest_point(pts, v, f, vert_mesh=torch.tensor([0, 1, 0, 1, 1, 1])),
                     lambda: meshdist.closest_point(pts, v, f, vert_mesh=torch.tensor([-1, 0, 0, 0, 0, 0])),
                     lambda: meshdist.signed_distance(pts, v, f, threshold=0.0), lambda: meshdist.signed_distance(pts, v, f, threshold=1.0)]
        for call in bad_calls:
            with pytest.raises(ValueError):
                call()


def test_fit_views_refuses_mesh_init_together_with_sphere_init(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fit_views
    base = ["--obj", "x.obj", "--tet_path", "t.npz", "--out", "o.pt"]
    with pytest.raises(SystemExit) as e:
        fit_views.main(base + ["--mesh_init", "--sphere_init", "0.5"])  # argparse's error, before anything is read or a GPU is asked for
    assert e.value.code == 2 and "exclude each other" in capsys.readouterr().err


def test_the_restatement_on_one_triangle_by_hand():
    tri = np.array([[(0, 0, 0), (4, 0, 0), (0, 4, 0)]], np.float32)
    want = {(-1, -1, 2): ((0, 0, 0), 6.0, "A"), (6, -1, 0): ((4, 0, 0), 5.0, "B"), (-1, 7, 0): ((0, 4, 0), 10.0, "C"),
            (2, -3, 0): ((2, 0, 0), 9.0, "AB"), (-2, 1, 0): ((0, 1, 0), 4.0, "AC"), (4, 4, 0): ((2, 2, 0), 8.0, "BC"),
            (1, 1, 3): ((1, 1, 0), 9.0, "interior"), (1, 2, -0.5): ((1, 2, 0), 0.25, "interior")}
    for dtype in (np.float32, np.float64):
        p = np.array(list(want), np.float32)
        d2, face, c = md.closest_restated(p, tri, dtype=dtype)
        for k, (q, (cw, dw, region)) in enumerate(want.items()):
            print(f"\n{np.dtype(dtype).name} {region}: query {q} -> {c[k].tolist()} d2 {d2[k]}")
            assert c[k].tolist() == list(cw) and d2[k] == dw and face[k] == 0 and d2.dtype == dtype, (region, dtype)
    # ties keep the lowest index, a NaN triangle is never taken, nothing taken gives +inf / -1 / the query
    two = np.concatenate([tri, tri])
    assert md.closest_restated(p, two)[1].tolist() == [0] * len(want)
    nan_first = np.concatenate([np.full((1, 3, 3), np.nan, np.float32), tri])
    d2n, fn, cn = md.closest_restated(p, nan_first)
    assert fn.tolist() == [1] * len(want) and np.array_equal(d2n, d2.astype(np.float32))
    d2e, fe, ce = md.closest_restated(p, nan_first[:1])
    assert np.isinf(d2e).all() and (fe == -1).all() and np.array_equal(ce, p)
    d2e, fe, ce = md.closest_restated(p, tri[:0])
    assert np.isinf(d2e).all() and (fe == -1).all() and np.array_equal(ce, p) and (md.winding_restated(p, tri[:0]) == 0).all()
    q = p.copy()
    q[2, 1] = np.nan                                                     # a NaN query takes nothing; the others are untouched
    d2q, fq, cq = md.closest_restated(q, tri)
    assert fq[2] == -1 and np.isinf(d2q[2]) and np.array_equal(np.delete(d2q, 2), np.delete(d2.astype(np.float32), 2))
    assert np.isnan(md.winding_restated(q, tri)[2]) and np.isfinite(np.delete(md.winding_restated(q, tri), 2)).all()
    # three equal corners: region A, the distance to the corner
    dot = np.full((1, 3, 3), 2.0, np.float32)
    d2d, fd, cd = md.closest_restated(np.zeros((1, 3), np.float32), dot)
    assert d2d[0] == 12.0 and fd[0] == 0 and cd[0].tolist() == [2, 2, 2]


def test_winding_numbers_of_closed_and_inward_wound_meshes():
    for name in md.CLOSED:
        w64, w32 = md.case_winding(name, np.float64), md.case_winding(name, np.float32)
        margin = float(np.abs(np.abs(w64) - 0.5).min())
        inside = int((np.abs(w64) >= 0.5).sum())
        print(f"\n{name}: min | |w| - 0.5 | {margin:.4f} inside {inside} of {w64.shape[0]} sign {np.sign(w64[np.abs(w64) >= 0.5]).mean():+.0f} "
              f"fp32 vs float64 {md.max_abs(w32, w64):.2e}")
        assert margin >= 0.49 and 0 < inside < w64.shape[0]
        assert np.array_equal(np.abs(w32) >= 0.5, np.abs(w64) >= 0.5) and w32.dtype == np.float32
        assert np.abs(np.abs(w64[np.abs(w64) >= 0.5]) - 1).max() < 1e-9 and np.abs(w64[np.abs(w64) < 0.5]).max() < 1e-9
    assert (md.case_winding("ptorus", np.float64)[np.abs(md.case_winding("ptorus", np.float64)) >= 0.5] < 0).all()      # wound inward
    v, f = rm.mesh("uvsphere")
    r = np.linalg.norm(md.lattice().astype(np.float64), axis=1)          # the faceted sphere lies between the radii 0.95 and 1
    w = np.abs(md.case_winding("uvsphere", np.float64))
    assert (w[r < 0.95] >= 0.5).all() and (w[r > 1.0] < 0.5).all() and (r < 0.95).sum() > 100


def test_the_fp32_restatement_picks_a_closest_triangle_of_float64():
    for name in md.CASES + (md.BIG,):
        tri, tri_ptr, _ = md.case_triangles(name)
        p, pm = md.queries(name, "lattice")
        _, face32, _ = md.case_closest(name, "lattice", np.float32)
        qptr = md.ptr_of(pm, md.n_meshes(name))
        worst = 0.0
        for m in range(md.n_meshes(name)):
            qs, ts = slice(qptr[m], qptr[m + 1]), slice(tri_ptr[m], tri_ptr[m + 1])
            d64 = md.dist2_matrix(p[qs], tri[ts], np.float64)
            picked = d64[np.arange(d64.shape[0]), face32[qs] - tri_ptr[m]]
            least = np.nanmin(d64, axis=1)
            assert (face32[qs] >= tri_ptr[m]).all() and (face32[qs] < tri_ptr[m + 1]).all(), name
            worst = max(worst, float((np.sqrt(picked) / np.sqrt(least)).max() - 1))
        print(f"\n{name}: the picked triangle's float64 distance over the float64 minimum - 1: {worst:.2e}")
        assert worst <= 1e-6, name


def test_gather_sorts_ungrouped_faces_stably_and_maps_back():
    v, f = rm.mesh("pair")
    vm = rm.vert_mesh("pair").numpy()
    perm = np.random.default_rng(3).permutation(f.shape[0])
    tri, ptr, face_of = md.gather(v.numpy(), f.numpy()[perm], vm)
    tri0, ptr0, face_of0 = md.case_triangles("pair")
    assert np.array_equal(ptr, ptr0) and np.array_equal(face_of0, np.arange(f.shape[0]))
    assert np.array_equal(tri, v.numpy()[f.numpy()[perm][face_of]]) and sorted(face_of.tolist()) == list(range(f.shape[0]))
    fm = vm[f.numpy()[perm][:, 0]]
    for m in range(2):                                                   # stable: the caller's order inside a mesh
        assert np.array_equal(face_of[ptr[m]:ptr[m + 1]], np.nonzero(fm == m)[0])


def test_projection_keeps_the_restated_remesh_on_its_input():
    for name in md.PROJECT_CASES:
        on, off = md.project_restated(name, True), md.project_restated(name, False)
        v, f = rm.mesh(name)
        plain = rm.remesh_restated(v.numpy(), f.numpy(), iters=md.PROJECT_ITERS, relax=0.5, vert_mesh=rm.vert_mesh(name).numpy())
        fig_on, fig_off = md.project_figures(name, *on[:3], on[3]["target"]), md.project_figures(name, *off[:3], off[3]["target"])
        print(f"\n{name}: with projection share {fig_on[0]:.3f} angle {fig_on[1]:.1f} distance mean {fig_on[2]:.2e} max {fig_on[3]:.2e}; "
              f"without {fig_off[0]:.3f} {fig_off[1]:.1f} {fig_off[2]:.2e} {fig_off[3]:.2e}; moved by at most "
              f"{[r['max_project_dist2'] ** 0.5 for r in on[3]['iterations']]}")
        assert all(np.array_equal(a, b) for a, b in zip(off[:3], plain[:3])) and off[3]["iterations"] == plain[3]["iterations"]
        assert all("max_project_dist2" in r for r in on[3]["iterations"]) and not any("max_project_dist2" in r for r in off[3]["iterations"])
        assert fig_on[3] < 1e-6 < fig_off[3] and rm.problems(on[1], on[0].shape[0], closed=name in rm.CLOSED) == []
    both, a, b = md.project_restated("pair", True), md.project_restated("ptorus", True), None
    assert np.array_equal(both[0][both[2] == 0], a[0]) and np.array_equal(both[1][:a[1].shape[0]], a[1])


def test_the_golden_file_regenerates_identically():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_meshdist
    path = os.path.join(GOLD, "meshdist.npz")
    gold, fresh = np.load(path), gen_golden_meshdist.generate()
    assert os.path.getsize(path) < 64 * 1024 and sorted(gold.files) == sorted(fresh) and all(gold[k].size == 1 for k in gold.files)
    for k in gold.files:
        assert gold[k] == fresh[k], k
    for name in md.CASES + (md.BIG,):
        assert 0 < float(gold[f"closest/{name}/lattice/unit_closest"]) < 1e-4 and 0 < float(gold[f"closest/{name}/lattice/unit_dist"]) < 1e-6, name
        assert 0 < float(gold[f"winding/{name}/unit"]) < 1e-6, name
    assert len(gold.files) == 4 * len(md.CASES) + 2 + len(md.CASES) + 1 + 10 * len(md.PROJECT_CASES)
