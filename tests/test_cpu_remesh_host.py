"""Host side of the isotropic remeshing (csrc/remesh.hip, meshdiffusion_amd/postprocess.py remesh) without a GPU: the export
tables, argument refusal through the loaded library, the numpy restatement of tests/remesh_cases.py against hand-made answers, the
validity checker on broken meshes and the recorded figures.  Each test prints its figures before it asserts."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import remesh_cases as rm
from conftest import GOLD, ROOT

NEW_EXPORTS = ("md_remesh_split_mark", "md_remesh_split_count", "md_remesh_split_emit", "md_remesh_collapse_candidates",
               "md_remesh_collapse_claim", "md_remesh_collapse_apply", "md_remesh_flip_candidates", "md_remesh_flip_claim",
               "md_remesh_flip_apply", "md_remesh_relax")


def test_new_exports_are_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import _lib, build, postprocess
    assert "remesh.hip" in build.SOURCES
    for macro, value, mine in (("MD_REMESH_COLLAPSE_ROUNDS", _lib.REMESH_COLLAPSE_ROUNDS, rm.COLLAPSE_ROUNDS),
                               ("MD_REMESH_FLIP_ROUNDS", _lib.REMESH_FLIP_ROUNDS, rm.FLIP_ROUNDS),
                               ("MD_REMESH_MAX_ITERS", _lib.REMESH_MAX_ITERS, rm.MAX_ITERS)):
        assert value == mine, macro
    assert (_lib.REMESH_COLLAPSE_ROUNDS, _lib.REMESH_FLIP_ROUNDS, _lib.REMESH_MAX_ITERS) == (8, 4, 32)
    src = open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "remesh.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "THE REMESHING CONTRACT" in src
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*float", src) and "unsafeAtomicAdd" not in src
    for name in ("remesh", "remesh_split", "remesh_collapse_round", "remesh_flip_round", "remesh_relax", "remesh_default_target"):
        assert callable(getattr(postprocess, name)), name


def test_new_exports_refuse_bad_arguments_without_a_gpu(hip_lib):
    from meshdiffusion_amd import _lib
    nul, one, odd = C.c_void_p(0), C.c_void_p(64), C.c_void_p(66)
    big = 1 << 40
    for name in NEW_EXPORTS:
        fn, types = getattr(hip_lib, name), _lib.SIGNATURES[name][1]
        ok = [one if t is C.c_void_p else (100 if t is C.c_int64 else 0.5) for t in types]
        ok[-1] = nul                                                     # the stream
        if name == "md_remesh_split_emit":
            ok[10] = 400                                                 # F_out >= F
        if name in ("md_remesh_split_emit", "md_remesh_relax"):          # the output may not be the input
            out = {"md_remesh_split_emit": 11, "md_remesh_relax": 11}[name]
            ok[out] = C.c_void_p(128)
            alias = list(ok); alias[out] = one
            assert fn(*alias) == -1, (name, "alias")
        pointers = [k for k, t in enumerate(types[:-1]) if t is C.c_void_p]
        sizes = [k for k, t in enumerate(types) if t is C.c_int64]
        for k in pointers:
            for bad in (nul, odd):
                a = list(ok); a[k] = bad
                assert fn(*a) == -1, (name, k, bad)
        for k in sizes:
            for bad in (0, -3):
                a = list(ok); a[k] = bad
                assert fn(*a) == -1, (name, k, bad)
            a = list(ok); a[k] = big
            if name == "md_remesh_split_emit":
                a[10] = max(a[10], a[9])
            assert fn(*a) == -2, (name, k, "beyond int32")
        for k, t in enumerate(types):
            if t is C.c_float:
                a = list(ok); a[k] = float("nan")
                assert fn(*a) == -1, (name, k, "nan")
    # 2 E and 3 F are what must fit int32
    ok = [one, one, one, one, 100, 1 << 30, 100, one, nul]
    assert hip_lib.md_remesh_split_count(*ok) == -2
    ok = [one, one, one, one, 100, 100, 1 << 30, one, nul]
    assert hip_lib.md_remesh_split_count(*ok) == -2


def test_python_entry_point_refuses_cpu_tensors_and_bad_arguments():
    from meshdiffusion_amd import _lib, postprocess
    v, f = rm.mesh("octa")
    with pytest.raises(_lib.MeshDiffusionHipError):
        postprocess.remesh(v, f)                                         # a CPU tensor: no fallback
    with pytest.raises(_lib.MeshDiffusionHipError):
        postprocess.postprocess([(v, f)], remesh_iters=1)
    if torch.cuda.is_available():
        v, f = v.cuda(), f.cuda()
        for kw in (dict(iters=33), dict(iters=-1), dict(target_len=0.0), dict(target_len=float("nan")), dict(target_len=float("inf")),
                   dict(target_scale=0.0), dict(target_len=[0.1, 0.2]), dict(relax=float("nan")), dict(flip_angle=120.0)):
            with pytest.raises(ValueError):
                postprocess.remesh(v, f, **kw)


def test_the_three_split_patterns_on_one_triangle():
    x = np.array([(0, 0, 0), (4, 0, 0), (0, 3, 0)], np.float32)          # edges (0,1) 4, (0,2) 3, (1,2) 5 in table order
    f, vm = np.array([[0, 1, 2]]), np.zeros(3, np.int32)
    want = {20.0: ([[0, 1, 3], [0, 3, 2]], [[2, 1.5, 0]]),                                              # bisect the longest
            10.0: ([[1, 4, 3], [4, 2, 0], [4, 0, 3]], [[2, 0, 0], [2, 1.5, 0]]),                         # corner + quad cut from the longer
            5.0: ([[0, 3, 4], [1, 5, 3], [2, 4, 5], [5, 4, 3]], [[2, 0, 0], [0, 1.5, 0], [2, 1.5, 0]])}   # one to four
    for hi2, (faces, new) in want.items():
        x2, f2, vm2, n = rm.split_restated(x, f, vm, np.array([hi2], np.float32))
        print(f"\nhi2 {hi2}: marked {n} faces {f2.tolist()} new vertices {x2[3:].tolist()}")
        assert f2.tolist() == faces and x2[3:].tolist() == new and n == len(new) and np.array_equal(x2[:3], x)
        area = [np.cross(x2[t[1]] - x2[t[0]], x2[t[2]] - x2[t[0]])[2] for t in f2]
        assert min(area) > 0 and abs(sum(area) - 12.0) < 1e-5            # every child keeps the orientation, the area is kept
        assert rm.problems(f2, x2.shape[0], closed=False) == []
    x2, f2, _, n = rm.split_restated(x, f, vm, np.array([25.0], np.float32))      # len2 == hi2 is not above it
    assert n == 0 and f2.tolist() == f.tolist()
    # the tie of the k = 2 pattern: the lower edge index cuts
    x = np.array([(0, 0, 0), (2, 0, 0), (1, 2, 0)], np.float32)          # (0,2) and (1,2) both sqrt 5
    _, f2, _, n = rm.split_restated(x, f, vm, np.array([4.5], np.float32))
    print(f"tie: {f2.tolist()}")
    assert n == 2 and f2.tolist() == [[2, 3, 4], [3, 0, 1], [3, 1, 4]]    # cut from the midpoint 3 of edge (0,2), index 1 < 2


def test_tetra_and_octa_never_collapse_into_a_double_face():
    for name in ("tetra", "octa"):
        v, f = rm.mesh(name)
        for scale in (1.0, 10.0):
            x, g, vm, info = rm.remesh_restated(v.numpy(), f.numpy(), iters=3, target_scale=scale)
            n = sum(r["collapses"] for r in info["iterations"])
            print(f"\n{name} x {scale}: collapses {n}, F {f.shape[0]} -> {g.shape[0]}, problems {rm.problems(g, x.shape[0])}")
            assert rm.problems(g, x.shape[0]) == [] and g.shape[0] >= 4 and rm.euler(g, vm, 1) == [2]
            if name == "tetra" or scale == 1.0:
                assert n == 0 and np.array_equal(g, f.numpy())           # valence three never collapses; nothing is short at scale 1
            else:
                assert n == 2 and g.shape[0] == 4                        # everything short: the octahedron ends as a tetrahedron and stops


def _canon(faces):
    return sorted(tuple(np.roll(t, -int(np.argmin(t)))) for t in np.asarray(faces).tolist())


def test_one_known_flip_on_a_valence_imbalanced_patch():
    v, f, even = rm.flip_patch()
    T = rm.tables(f, v.shape[0])
    val = T["ptr"][1:] - T["ptr"][:-1]
    print(f"\nvalences around the middle cell: {[int(val[i]) for i in (14, 15, 20, 21)]}")
    assert [int(val[i]) for i in (14, 15, 20, 21)] == [5, 7, 7, 5]
    out, n = rm.flip_round_restated(v, f, rm.cos2_of(30.0))
    changed = np.nonzero((out != f).any(1))[0].tolist()
    print(f"winners {n}, slots rewritten {changed}: {out[changed].tolist()}")
    assert n == 1 and sorted(out[changed].tolist()) == [[14, 20, 21], [15, 14, 21]]
    assert _canon(out) == _canon(even) and rm.problems(out, v.shape[0], closed=False) == []
    again, n = rm.flip_round_restated(v, out, rm.cos2_of(30.0))
    assert n == 0 and np.array_equal(again, out)                         # the balanced grid is a fixed point
    long = v.copy()                                                      # stretched along (1, 1): the middle cell's diagonal is now the short one
    long[:, :2] = v[:, :2] + (v[:, :1] + v[:, 1:2])                       # (x, y) -> (2x + y, x + 2y): eigenvalues 3 along (1, 1), 1 across
    q0, q1 = rm.quality(long, f[24:26], 1.0)[1], rm.quality(long, even[24:26], 1.0)[1]      # the middle cell's two faces
    print(f"stretched: minimum angle with the short diagonal {q0:.1f}, after the valence flip it would be {q1:.1f}")
    assert q1 < q0 and rm.flip_round_restated(long, f, rm.cos2_of(30.0))[1] == 0      # same valences, but the flip would lower the smallest angle
    bent = v.copy()
    bent[21, 2] = 2.0                                                    # the two faces now meet at more than 30 degrees
    assert rm.flip_round_restated(bent, f, rm.cos2_of(30.0))[1] == 0


def test_the_validity_checker_on_deliberately_broken_meshes():
    v, f = rm.mesh("tetra")
    f = f.numpy()
    assert rm.problems(f, 4) == [] and rm.euler(f, np.zeros(4, np.int64), 1) == [2]
    cases = {"a face removed": (f[:3], 4, "mult != 2"), "a face turned over": (np.concatenate([f[:3], f[3:, [0, 2, 1]]]), 4, "duplicate directed"),
             "a face twice": (np.concatenate([f, f[:1]]), 4, "mult != 2"), "an unused vertex": (f, 5, "unreferenced"),
             "a repeated index": (np.concatenate([f, [[0, 0, 1]]]), 4, "degenerate"),
             "two tetrahedra sharing a vertex": (np.concatenate([f, np.where(f == 0, 0, f + 3)]), 7, "vertex 0: fan"),
             "an index out of range": (f + 1, 4, "out of range")}
    for tag, (faces, V, word) in cases.items():
        got = rm.problems(faces, V)
        print(f"\n{tag}: {got}")
        assert any(word in p for p in got), tag
    assert rm.problems(f[:3], 4, closed=False) == []                     # an open mesh is fine where a boundary is allowed
    for name in rm.CASES:
        if name not in ("degen",):
            v, f = rm.mesh(name)
            assert rm.problems(f.numpy(), v.shape[0], closed=name in rm.CLOSED) == [], name
    v, f = rm.mesh("uvsphere")
    assert (v.shape[0], f.shape[0]) == (266, 528) and rm.tables(f.numpy(), 266)["lo"].shape[0] == 792
    assert rm.euler(rm.mesh("pair")[1].numpy(), rm.vert_mesh("pair").numpy(), 2) == [0, 1]


def test_the_restated_pipeline_keeps_every_case_valid():
    for name in ("uvsphere", "ptorus", "pair", "fan40", "quad", "degen"):
        v, f = rm.mesh(name)
        vm = rm.vert_mesh(name).numpy()
        M = int(vm.max()) + 1
        x, g, vm2, info = rm.pipeline_restated(name, 1.0, 0.5, 2)
        proper = g[~rm.repeated(g)]
        bad = [p for p in rm.problems(proper, x.shape[0], closed=name in rm.CLOSED) if name not in ("degen",) or "unreferenced" not in p]
        print(f"\n{name}: V {v.shape[0]} -> {x.shape[0]} F {f.shape[0]} -> {g.shape[0]} chi {rm.euler(g, vm2, M)} per iteration "
              f"{[tuple(r.values()) for r in info['iterations']]} problems {bad}")
        assert bad == [] and np.isfinite(x).all() and bool((np.diff(vm2) >= 0).all())
        if name != "degen":
            assert rm.euler(g, vm2, M) == rm.euler(f.numpy(), vm, M)
    both = rm.pipeline_restated("pair", 1.0, 0.5, 2)                     # the batch equals its halves, index offsets aside
    a, b = rm.pipeline_restated("ptorus", 1.0, 0.5, 2), rm.pipeline_restated("fan40", 1.0, 0.5, 2)
    assert np.array_equal(both[0], np.concatenate([a[0], b[0]])) and np.array_equal(both[1], np.concatenate([a[1], b[1] + a[0].shape[0]]))


def test_the_golden_file_regenerates_identically():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_remesh
    path = os.path.join(GOLD, "remesh.npz")
    gold, fresh = np.load(path), gen_golden_remesh.generate()
    assert os.path.getsize(path) < 64 * 1024 and sorted(gold.files) == sorted(fresh) and all(gold[k].size == 1 for k in gold.files)
    for k in gold.files:
        assert gold[k] == fresh[k], k
    for name in rm.EXACT_CASES:
        assert 0 < float(gold[f"relax/{name}/ref_err"]) < 1e-6, name
    assert 0 < float(gold["fidelity/uvsphere/radial_dev"]) < 0.05
    assert len(gold.files) == len(rm.EXACT_CASES) + 5 * len(rm.QUALITY_CASES) + 1
