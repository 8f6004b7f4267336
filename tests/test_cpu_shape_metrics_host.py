"""Generation metrics, host side (no GPU): the new export and its argument checks, the float64 restatements of
tests/shape_metrics_cases.py against hand-written answers, `normalize_clouds`, and the INPUT CONDITIONS the GPU tests rely on
-- proven here in float64 so that an fp32 matrix within the value bar cannot flip an argmin."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import shape_metrics_cases as sm
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_new_export_is_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import build, metrics
    assert "shape_metrics.hip" in build.SOURCES
    for name in ("sided_mean_matrix", "chamfer_matrix", "mmd_cov", "one_nna", "shape_metrics", "normalize_clouds",
                 "clouds_from_meshes"):
        assert callable(getattr(metrics, name)), name


def _refuses(fn, ok, pointers, sizes):
    """-1 for each of `pointers` set to null and each of `sizes` set to 0 or a negative number; `ok` ends with a null stream."""
    nul = C.c_void_p(0)
    assert ok[-1].value is None
    for k in pointers:
        a = list(ok)
        a[k] = nul
        assert fn(*a) == -1, (fn.__name__, k)
    for k in sizes:
        for bad in (0, -3):
            a = list(ok)
            a[k] = bad
            assert fn(*a) == -1, (fn.__name__, k, bad)


def test_new_export_refuses_bad_arguments_without_a_gpu(hip_lib):
    nul, one = C.c_void_p(0), C.c_void_p(64)
    # md_sided_mean_matrix(x, y, nx, ny, p, q, out, stream)
    _refuses(hip_lib.md_sided_mean_matrix, [one, one, 3, 5, 7, 11, one, nul], (0, 1, 6), (2, 3, 4, 5))
    assert hip_lib.md_sided_mean_matrix(one, one, 1 << 24, 5, 7, 11, one, nul) == -2      # 2^24 workgroups of 256 lanes along x


def test_host_functions_refuse_cpu_tensors_and_wrong_ranks():
    from meshdiffusion_amd import _lib, metrics
    x = torch.zeros(2, 4, 3)
    for call in (lambda: metrics.sided_mean_matrix(x, x), lambda: metrics.chamfer_matrix(x), lambda: metrics.chamfer_matrix(x, x),
                 lambda: metrics.shape_metrics(x, x)):
        with pytest.raises(_lib.MeshDiffusionHipError):
            call()
    with pytest.raises(ValueError):
        metrics.mmd_cov(torch.zeros(3))
    with pytest.raises(ValueError):
        metrics.one_nna(torch.zeros(2, 2), torch.zeros(2, 3), torch.zeros(2, 2))
    with pytest.raises(ValueError):
        metrics.normalize_clouds(x, "sphere")


# d_sr, samples by references.  Row minima: s0 -> r1 (1), s1 -> r0 (2, tie with r2: the lowest), s2 -> r1 (0.5)
D3 = [[4.0, 1.0, 3.0], [2.0, 5.0, 2.0], [6.0, 0.5, 7.0]]
# column minima 2, 0.5, 2 -> mmd 1.5; covered references {0, 1} -> 2/3
# 4 x 4: every sample's nearest reference is r3 except s3 (tie r0 = r2 = 1 -> r0): covered {0, 3} -> 0.5; column minima 1, 2, 1, 0.25
D4 = [[3.0, 2.0, 3.0, 0.25], [5.0, 4.0, 6.0, 1.0], [7.0, 8.0, 9.0, 2.0], [1.0, 2.0, 1.0, 3.0]]


def test_mmd_cov_on_hand_written_matrices():
    from meshdiffusion_amd import metrics
    for fn in (sm.mmd_cov_restated, metrics.mmd_cov):
        mmd, cov = fn(torch.tensor(D3))
        assert mmd == 1.5 and cov == 2 / 3, fn
        mmd, cov = fn(torch.tensor(D4))
        assert mmd == (1 + 2 + 1 + 0.25) / 4 and cov == 0.5, fn
        mmd, cov = fn(torch.tensor(D3, dtype=torch.float32).t().contiguous())      # [R,S] read as [S,R]: rows -> r1, r2, r1
        assert mmd == (1 + 2 + 0.5) / 3 and cov == 2 / 3, fn


def test_one_nna_on_hand_written_matrices():
    from meshdiffusion_amd import metrics
    # union s0 s1 s2 r0 r1 r2.  Nearest other (diagonal excluded):
    #   s0: ss (., 9, 8) sr (4, 1, 3) -> r1, wrong       s1: ss (9, ., 1.5) sr (2, 5, 2) -> s2, right
    #   s2: ss (8, 1.5, .) sr (6, 0.5, 7) -> r1, wrong   r0: column 0 of sr (4, 2, 6), rr (., 2, 9) -> tie s1 = r1 = 2 -> s1, wrong
    #   r1: (1, 5, 0.5), (2, ., 0.1) -> r2, right        r2: (3, 2, 7), (9, 0.1, .) -> r1, right
    d_ss = torch.tensor([[0.0, 9.0, 8.0], [9.0, 0.0, 1.5], [8.0, 1.5, 0.0]])
    d_rr = torch.tensor([[0.0, 2.0, 9.0], [2.0, 0.0, 0.1], [9.0, 0.1, 0.0]])
    for fn in (sm.one_nna_restated, metrics.one_nna):
        assert fn(d_ss, torch.tensor(D3), d_rr) == (3 / 6, 1 / 3, 2 / 3), fn
    # 4 + 4: two families far apart -> 1.0; the same set on both sides (d_sr = d_ss) -> every nearest other is the twin -> 0.0
    near = torch.tensor([[0.0, 1.0, 2.0, 3.0], [1.0, 0.0, 1.5, 2.5], [2.0, 1.5, 0.0, 1.0], [3.0, 2.5, 1.0, 0.0]])
    far = near + 50.0
    for fn in (sm.one_nna_restated, metrics.one_nna):
        assert fn(near, far, near) == (1.0, 1.0, 1.0), fn
        assert fn(near, near, near) == (0.0, 0.0, 0.0), fn
    # a diagonal that is not the minimum-by-being-zero still never votes: all entries equal -> lowest OTHER index
    flat = torch.ones(4, 4)
    for fn in (sm.one_nna_restated, metrics.one_nna):
        # s0 -> s1 right, s1..s3 -> s0 right; r0..r3 -> s0 wrong
        assert fn(flat, flat, flat) == (0.5, 1.0, 0.0), fn
    with pytest.raises(ValueError):
        metrics.one_nna(torch.zeros(1, 1), torch.zeros(1, 0), torch.zeros(0, 0))


def test_normalize_clouds_on_a_known_box():
    from meshdiffusion_amd.metrics import normalize_clouds
    corners = torch.tensor([[1.0, 2.0, 3.0], [5.0, 4.0, 4.0], [3.0, 3.0, 3.5]])      # box [1,5] x [2,4] x [3,4]: centre (3,3,3.5), side 4
    pts = torch.stack([corners, corners * 2 + 7])
    out = normalize_clouds(pts, "bbox")
    want = torch.tensor([[-0.5, -0.25, -0.125], [0.5, 0.25, 0.125], [0.0, 0.0, 0.0]])
    assert torch.equal(out[0], want) and torch.equal(out[1], want)
    assert normalize_clouds(pts, "none") is pts
    with pytest.raises(ValueError):
        normalize_clouds(torch.ones(1, 4, 3), "bbox")


def test_value_bar_constant_and_lattice_expectations():
    assert sm.VALUE_BAR == 18 * 2.0 ** -24 and sm.ARGMIN_GAP == 2.0 ** -18 and sm.CONSISTENCY_BAR == 2.0 ** -23
    x, y = sm.case("lattice")
    assert x.shape == (3, 512, 3) and y.shape == (2, 512, 3)
    for t in (x, y):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 42      # squares <= 42^2 * 3 < 2^24: every fp32 step exact
    assert sm.sided_mean_float64(x, y).tolist() == sm.LATTICE_EXPECTED
    assert sm.sided_mean_fp32(x, y).tolist() == sm.LATTICE_EXPECTED


def test_case_shapes_and_run_lengths():
    shapes = {"tiny": (3, 5, 7, 11), "ones": (2, 2, 1, 1), "edges": (2, 3, 2049, 1025), "typical": (6, 7, 2048, 2048),
              "near": (3, 3, 2048, 2048), "offset": (3, 3, 2048, 2048), "runs": (1, 70, 64, 64), "self": (9, 9, 2048, 2048),
              "lattice": (3, 2, 512, 512), "run3": (300, 20, 33, 17), "run2_blocks": (1100, 3, 2049, 5),
              "run_tail": (256, 40, 9, 1027)}
    assert set(shapes) == set(sm.FINITE_CASES)
    run_len = lambda nx, ny: -(-ny // min(ny, -(-2048 // nx)))          # noqa: E731   the launch's run length (shape_metrics.hip)
    for name, (nx, ny, p, q) in shapes.items():
        x, y = sm.case(name)
        assert x.shape == (nx, p, 3) and y.shape == (ny, q, 3) and x.dtype == torch.float32 and y.dtype == torch.float32, name
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all()), name
    x, y = sm.case("self")
    assert x is y
    assert [run_len(*shapes[n][:2]) for n in ("run3", "run2_blocks", "run_tail")] == [3, 2, 5]
    assert all(run_len(*shapes[n][:2]) == 1 for n in sm.FINITE_CASES[:9])
    x, y, cx, cy = sm.nonfinite_case()
    tx, ty = sm.case("tiny")
    assert x.shape == (4, 7, 3) and y.shape == (6, 11, 3)
    assert all(torch.equal(x[i], tx[i]) for i in cx) and all(torch.equal(y[j], ty[j]) for j in cy)
    want = sm.sided_mean_fp32(x, y)
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isnan(want[3, 5]))          # the NaN cloud; inf - inf
    assert bool(torch.isinf(want[3, [0, 1, 3, 4]]).all()) and bool(torch.isnan(want[3, 2]))      # inf from finite clouds; inf - inf again
    assert bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[2]).all())     # an infinite candidate never wins


def test_input_conditions_non_finite_points_lie_outside_the_last_tile():
    for name in sm.NONFINITE_TILE_CASES:
        x, y, clean = sm.nonfinite_tile_case(name)
        q = y.shape[1]
        bad = (~torch.isfinite(y[0])).any(dim=1).nonzero().flatten()
        assert q > 1024 and len(bad) == 1 and int(bad[0]) < (q - 1) // 1024 * 1024, name          # finite tiles follow it
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y[1]).all()) and torch.equal(y[1], clean[1]), name
        want = sm.sided_mean_fp32(x, y)
        assert bool(torch.isnan(want[:, 0]).all()) and bool(torch.isfinite(want[:, 1]).all()), name
    assert sm.nonfinite_tile_case("nan_middle_tile")[1].shape[1] > 2048 and sm.nonfinite_tile_case("nan_blocks")[0].shape[1] > 2048


def test_fp32_direct_form_has_room_under_the_value_bar():
    for name in ("tiny", "edges", "typical", "near", "offset"):
        x, y = sm.case(name)
        ok, worst = sm.within_bar(sm.sided_mean_fp32(x, y), sm.sided_mean_float64(x, y))
        print(f"{name}: torch fp32 direct form worst relative error {worst:.2e} = {worst / sm.VALUE_BAR:.3f} of the bar")
        assert ok and worst < 0.25 * sm.VALUE_BAR, name


@pytest.mark.parametrize("name", sm.METRIC_CASES)
def test_input_conditions_metric_argmins_are_well_separated(name):
    """Every row minimum COV and 1-NNA use is separated from its runner-up by a relative gap > 2^-18 in float64 ("identical":
    apart from the exact zero of a cloud against its twin, which fp32 reproduces exactly)."""
    sm_meshes, ref_meshes, us, ur = sm.metric_meshes(name)
    s = sm.clouds_restated(sm_meshes, us)
    r = s if name == "identical" else sm.clouds_restated(ref_meshes, ur)
    S = s.shape[0]
    d_ss = sm.chamfer_float64(s)
    d_sr, d_rr = (d_ss, d_ss) if name == "identical" else (sm.chamfer_float64(s, r), sm.chamfer_float64(r))
    gap = sm.argmin_gaps(d_ss, d_sr, d_rr)
    mmd, cov = sm.mmd_cov_restated(d_sr)
    nna = sm.one_nna_restated(d_ss, d_sr, d_rr)
    print(f"{name}: smallest relative argmin gap {gap:.3e} (needed > {sm.ARGMIN_GAP:.3e}); mmd {mmd:.6e} cov {cov} 1-nna {nna}")
    assert gap > sm.ARGMIN_GAP, name
    if name == "identical":
        assert mmd == 0 and cov == 1 and nna == (0.0, 0.0, 0.0)
        off = d_ss[~torch.eye(S, dtype=torch.bool)]
        assert float(off.min()) > 0                                   # only a twin is at distance zero
    if name == "families":
        assert nna == (1.0, 1.0, 1.0)
        assert float(d_sr.min()) > 4 * max(float(d_ss.max()), float(d_rr.max()))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_kernel_uses_no_scratch_and_no_matrix_core(tmp_path):
    csrc = os.path.join(ROOT, "meshdiffusion_amd", "csrc")
    out = tmp_path / "shape_metrics.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{ROOT}/include",
                    f"-I{csrc}", os.path.join(csrc, "shape_metrics.hip"), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    text = out.read_text()
    seen = []
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))      # noqa: E731
        assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
        seen.append(name)
    assert any("md_sided_mean_matrix_kernel" in n for n in seen), seen
    assert "v_mfma" not in text
