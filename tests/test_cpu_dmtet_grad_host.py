"""Differentiable marching tetrahedra, host side (no GPU): the three new exports, the static incidence list, the float64
restatement against the reference gradients of tests/golden/dmtet_grad.npz, and the ISA budget of the new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dmtet_grad_cases as dg
from conftest import GOLD, ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def tet():
    t = np.load(os.path.join(GOLD, "64_tets_cropped.npz"))
    return t["vertices"], t["indices"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "dmtet_grad.npz"))


def test_new_exports_are_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import _lib, build
    assert _lib.SDF_REG_SLABS == 64 and _lib.SDF_REG_WORKSPACE_BYTES == 24 * 64
    assert "dmtet_bwd.hip" in build.SOURCES


def test_new_exports_refuse_bad_arguments_without_a_gpu(hip_lib):
    nul, one = C.c_void_p(0), C.c_void_p(64)
    bwd = hip_lib.md_marching_tets_bwd
    ok = [one] * 8 + [2, 100, 300, one, one, nul]
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 11, 12):                    # every pointer but the stream
        a = list(ok)
        a[k] = nul
        assert bwd(*a) == -1, k
    for k in (8, 9, 10):                                           # n_meshes, n_verts, n_edges
        for bad in (0, -3):
            a = list(ok)
            a[k] = bad
            assert bwd(*a) == -1, (k, bad)
    a = list(ok)
    a[8] = 70000                                                   # gridDim.y
    assert bwd(*a) == -2
    fwd = hip_lib.md_sdf_reg_loss
    ok = [one, one, 100, 300, one, one, one, nul]
    for k in (0, 1, 4, 5, 6):
        a = list(ok)
        a[k] = nul
        assert fwd(*a) == -1, k
    for k in (2, 3):
        for bad in (0, -1):
            a = list(ok)
            a[k] = bad
            assert fwd(*a) == -1, (k, bad)
    assert fwd(one, C.c_void_p(68), 100, 300, one, one, one, nul) == -1          # edge rows are read as 8-byte pairs
    rb = hip_lib.md_sdf_reg_loss_bwd
    ok = [one] * 6 + [100, 300, one, nul]
    for k in (0, 1, 2, 3, 4, 5, 8):
        a = list(ok)
        a[k] = nul
        assert rb(*a) == -1, k
    for k in (6, 7):
        for bad in (0, -1):
            a = list(ok)
            a[k] = bad
            assert rb(*a) == -1, (k, bad)


def test_incidence_list_of_the_shipped_grid(tet):
    from meshdiffusion_amd.dmtet import TetTables
    verts, idx = tet
    tb = TetTables(idx, "cpu")
    assert not tb._incidence                                        # lazy: nothing is built before a gradient is needed
    N, E = verts.shape[0], tb.n_edges
    inc_ptr, inc = tb.incidence(N)
    assert inc_ptr.dtype == torch.int32 and inc.dtype == torch.int32
    assert inc_ptr.shape == (N + 1,) and inc.shape == (2 * E,) and int(inc_ptr[0]) == 0 and int(inc_ptr[-1]) == 2 * E
    deg = (inc_ptr[1:] - inc_ptr[:-1]).long()
    assert int(deg.max()) == 14 and int(deg.min()) >= 1 and abs(float(deg.float().mean()) - 12.8) < 0.05
    # every edge exactly twice, once per endpoint
    assert torch.equal(torch.sort(inc.long())[0], torch.arange(2 * E))
    owner = torch.repeat_interleave(torch.arange(N), deg)
    e, side = (inc >> 1).long(), (inc & 1).long()
    assert torch.equal(tb.edges.long()[e, side], owner)             # the entry's endpoint IS the vertex it is listed under
    # ascending edge id inside a vertex: e may only fall where the owner changes
    fall = e[1:] <= e[:-1]
    assert bool((owner[1:] != owner[:-1])[fall].all())
    assert tb.incidence(N)[1] is inc                                # cached
    with pytest.raises(ValueError):
        TetTables(idx, "cpu").incidence(N - 1)                      # an edge table that names a vertex the arrays do not have
    assert torch.equal(tb.all_edges, dg.unique_edges(idx)) and tb.all_edges._md_tables is tb


def test_float64_restatement_reproduces_the_reference_gradients(tet, gold):
    """Build-host pin of tests/dmtet_grad_cases.py: on the fixture's stored rows the restatement is as close to the
    reference as the generator recorded for the whole case (x 2: a subset's rel-L2 scatters around the whole's)."""
    from oracle.gen_golden import dmtet_cases
    verts, idx = tet
    pos, cases = dmtet_cases(verts)
    edges = dg.unique_edges(idx)
    N = pos.shape[0]
    for name in dg.GRAD_CASES:
        V, sdf = int(gold[f"{name}/V"]), cases[name]
        assert dg.crossing_edges(sdf, edges).shape[0] == V
        dpos, dsdf = dg.restated_grads(pos, sdf, edges, dg.case_G(V, gold[f"{name}/seed"]))
        rows, rp, rs = dg.fixture_rows(gold, name, N)
        ep, es = dg.rel_l2(rp, dpos[rows]), dg.rel_l2(rs, dsdf[rows])
        print(f"{name}: reference rows vs float64 dpos {ep:.2e} (recorded {float(gold[f'{name}/ref_err_dpos']):.2e}) "
              f"dsdf {es:.2e} (recorded {float(gold[f'{name}/ref_err_dsdf']):.2e})")
        assert ep <= 2 * float(gold[f"{name}/ref_err_dpos"]) and es <= 2 * float(gold[f"{name}/ref_err_dsdf"]), name
        zp, zs = dg.fixture_zero_rows(gold, name, N)
        assert bool((dpos[zp] == 0).all()) and bool((dsdf[zs].abs() <= 1e-12 * dsdf.abs().max()).all()), name
        if name == "noise":
            assert np.abs(dpos.sum(0).numpy() - gold["noise/dpos_colsum"]).max() <= 1e-5 * float(dpos.abs().sum(0).max())
            assert abs(float(dsdf.sum()) - float(gold["noise/dsdf_sum"])) <= 1e-5 * float(dsdf.abs().sum())
    for name in dg.REG_CASES:
        loss, g = dg.restated_sdf_reg(cases[name], edges)
        assert abs(float(loss) - float(gold[f"reg/{name}/value64"])) <= 1e-12 * abs(float(loss))
        assert abs(float(loss) - float(gold[f"reg/{name}/value"])) <= max(2 * float(gold[f"reg/{name}/ref_err_value"]), 2.0 ** -24) * float(loss)
        rows = gold[f"reg/{name}/rows"].astype(np.int64)
        assert dg.rel_l2(gold[f"reg/{name}/grad"], g[rows]) <= 2 * float(gold[f"reg/{name}/ref_err_grad"]), name
        assert int((g != 0).sum()) == int(gold[f"reg/{name}/n_nonzero"])


def test_fixture_is_small_and_carries_the_fit(gold):
    assert os.path.getsize(os.path.join(GOLD, "dmtet_grad.npz")) < 1 << 20
    assert list(gold["fit/steps"]) == list(dg.FIT_STEPS) and int(gold["fit/V0"]) > 0
    l32, l64 = gold["fit/loss32"], gold["fit/loss64"]
    assert l32[3] <= 0.01 * l32[0] and np.abs(l32 - l64).max() <= 1e-3 * l64.max()
    for name in dg.GRAD_CASES:
        assert 0 < float(gold[f"{name}/ref_err_dpos"]) < 1e-6 and 0 < float(gold[f"{name}/ref_err_dsdf"]) < 5e-6


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernels_use_no_scratch(tmp_path):
    csrc = os.path.join(ROOT, "meshdiffusion_amd", "csrc")
    out = tmp_path / "dmtet_bwd.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{ROOT}/include",
                    f"-I{csrc}", os.path.join(csrc, "dmtet_bwd.hip"), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    text = out.read_text()
    seen = set()
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))      # noqa: E731
        assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
        assert get("vgpr_count") <= 64, name                        # latency-bound gathers: full occupancy
        seen.add(name)
    for k in ("md_mt_bwd_kernel", "md_sdf_reg_partial_kernel", "md_sdf_reg_final_kernel", "md_sdf_reg_bwd_kernel"):
        assert any(k in n for n in seen), (k, seen)
    assert "scratch_" not in text and "global_atomic" not in text and "flat_atomic" not in text
