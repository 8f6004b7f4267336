"""Earth mover's distance and JSD, host side (no GPU): the new export and its argument checks, `emd_quantum` and `jsd` against
hand-made answers, the restatements of tests/emd_cases.py against each other, and the DERIVED BARS of that file shown to hold
for scipy on the kernel's integer matrix on every finite case -- so that what the GPU test asks of the kernel is what exact
arithmetic on that matrix achieves."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import emd_cases as ec
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_emd_export_is_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import build, metrics
    header = open(os.path.join(ROOT, "include", "meshdiffusion_hip.h")).read()
    assert "THE EMD CONTRACT" in header
    assert "emd.hip" in build.SOURCES
    for name in ("emd_quantum", "emd_matrix", "jsd", "shape_metrics"):
        assert callable(getattr(metrics, name)), name
    assert metrics.EMD_MAX_POINTS == ec.MAX_P


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


def test_emd_export_refuses_bad_arguments_without_a_gpu(hip_lib):
    nul, one, two = C.c_void_p(0), C.c_void_p(64), C.c_void_p(128)
    fn = hip_lib.md_emd_matrix
    # md_emd_matrix(x, y, nx, ny, p, quantum, max_rounds, triangular, out, status, total, rounds, perm, stream)
    ok = [one, two, 3, 5, 7, 2.0 ** -20, 100, 0, one, one, nul, nul, nul, nul]
    _refuses(fn, ok, (0, 1, 8, 9), (2, 3, 4, 6))                 # x, y, out, status; nx, ny, p, max_rounds
    for quantum in (0.0, 3.0, float("nan"), -0.5, float("inf"), 2.0 ** -20 * 1.5):
        a = list(ok)
        a[5] = quantum
        assert fn(*a) == -1, quantum
    for p, want in ((2049, -2), (1 << 20, -2)):                  # both clouds of a pair live in LDS
        a = list(ok)
        a[4] = p
        assert fn(*a) == want, p
    a = list(ok)
    a[2], a[3] = 1 << 16, 1 << 15                                # nx * ny = 2^31 workgroups
    assert fn(*a) == -2
    tri = [one, one, 5, 5, 7, 2.0 ** -20, 100, 1, one, one, nul, nul, nul, nul]
    for k, v in ((2, 4), (3, 6), (1, two)):                      # triangular: nx != ny, x != y
        a = list(tri)
        a[k] = v
        assert fn(*a) == -1, (k, v)


def test_emd_host_functions_refuse_cpu_tensors_and_wrong_shapes():
    from meshdiffusion_amd import _lib, metrics
    x = torch.zeros(2, 4, 3)
    for call in (lambda: metrics.emd_matrix(x), lambda: metrics.emd_matrix(x, x.clone()),
                 lambda: metrics.shape_metrics(x, x, emd=True), lambda: metrics.shape_metrics(x, x, jsd=True)):
        with pytest.raises(_lib.MeshDiffusionHipError):
            call()
    # emd_matrix looks at the shapes before it looks at the device: the limits are named without a GPU
    with pytest.raises(ValueError, match="2048"):
        metrics.emd_matrix(torch.zeros(1, 2049, 3))
    with pytest.raises(ValueError, match="same number of points, got 4 and 5"):
        metrics.emd_matrix(x, torch.zeros(3, 5, 3))
    for bad in (torch.zeros(4, 3), torch.zeros(2, 4, 2), torch.zeros(0, 4, 3), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError, match="N,P,3"):
            metrics.emd_matrix(bad)
        with pytest.raises(ValueError, match="N,P,3"):
            metrics.emd_matrix(x, bad)
    with pytest.raises(ValueError):
        metrics.jsd(torch.zeros(2, 4, 2), x)
    with pytest.raises(ValueError):
        metrics.jsd(x, torch.zeros(0, 4, 3))
    for bad in (float("nan"), float("inf")):
        y = x.clone()
        y[1, 2, 0] = bad
        with pytest.raises(ValueError, match="non-finite"):
            metrics.jsd(x, y)
        with pytest.raises(ValueError, match="non-finite"):
            metrics.jsd(y, x)
    with pytest.raises(ValueError):
        metrics.emd_quantum()


def test_emd_quantum_on_hand_made_boxes():
    from meshdiffusion_amd.metrics import emd_quantum
    box = lambda *corner: torch.tensor([[0.0, 0.0, 0.0], list(corner)])          # noqa: E731
    # diagonal 5 (3-4-0): ceil(log2 5) = 3
    assert emd_quantum(box(3.0, 4.0, 0.0)) == 2.0 ** (3 - 20)
    assert emd_quantum(box(3.0, 4.0, 0.0), bits=8) == 2.0 ** (3 - 8)
    # an exact power of two stays: diagonal 4 -> 2, diagonal 0.25 -> -2; just above it goes up
    assert emd_quantum(box(0.0, 4.0, 0.0)) == 2.0 ** (2 - 20)
    assert emd_quantum(box(0.25, 0.0, 0.0)) == 2.0 ** (-2 - 20)
    assert emd_quantum(box(0.0, 4.0, 2.0 ** -10)) == 2.0 ** (3 - 20)
    # the unit cube: sqrt 3 -> 1
    assert emd_quantum(box(1.0, 1.0, 1.0)) == 2.0 ** (1 - 20)
    # the box of ALL clouds: [0,3] x [0,0] x [0,0] and [0,0] x [-4,0] x [0,0] -> diagonal 5
    assert emd_quantum(box(3.0, 0.0, 0.0)[None], box(0.0, -4.0, 0.0)[None]) == 2.0 ** (3 - 20)
    # no extent
    assert emd_quantum(torch.ones(3, 5, 3)) == 2.0 ** -20
    for name in ec.EXACT_CASES + ec.FINITE_CASES:
        x, y = ec.case(name)
        assert emd_quantum(x, y) == ec.quantum_restated(x, y), name


def test_jsd_on_hand_computed_histograms():
    from meshdiffusion_amd.metrics import jsd
    res = 4                                                      # cells of side 0.25: cell index floor((c + 0.5) * 4)
    pt = lambda *c: list(c)                                      # noqa: E731
    a = torch.tensor([[pt(-0.4, -0.4, -0.4), pt(0.1, 0.1, 0.1)], [pt(0.3, -0.3, 0.2), pt(-0.1, 0.4, 0.0)]])
    assert jsd(a, a.clone(), res) == 0.0                         # identical sets
    assert jsd(a, a[:, [1, 0]][[1, 0]], res) == 0.0              # the order of clouds and points does not enter
    # disjoint cells: all of P in cell (0,0,0), all of Q in cell (3,3,3) -> H(M) = 1, H(P) = H(Q) = 0
    p = torch.full((1, 5, 3), -0.45)
    q = torch.full((2, 3, 3), 0.45)
    assert jsd(p, q, res) == 1.0
    # two cells A, B.  P = (3/4, 1/4), Q = (1/4, 3/4): M = (1/2, 1/2), H(M) = 1;
    # H(P) = H(Q) = -(3/4 log2 3/4 + 1/4 log2 1/4) = 2 - 3/4 log2 3 = 0.8112781244591328;  JSD = 1 - H(P) = 0.18872187554086717
    A, B = pt(-0.45, -0.45, -0.45), pt(0.45, 0.45, 0.45)
    p = torch.tensor([[A, A, A, B]])
    q = torch.tensor([[A, B], [B, B]])
    assert abs(jsd(p, q, res) - (0.75 * np.log2(3) - 1)) < 1e-15
    assert abs(jsd(p, q, res) - 0.18872187554086717) < 1e-15
    assert jsd(p, q, res) == jsd(q, p, res)
    # a point exactly on +0.5 would be cell `res`: it is clamped into the last cell, as -0.5 is the first and points outside are
    edge = torch.tensor([[pt(0.5, 0.5, 0.5), pt(-0.5, -0.5, -0.5), pt(0.7, 0.9, 2.0)]])
    inside = torch.tensor([[pt(0.49, 0.49, 0.49), pt(-0.49, -0.49, -0.49), pt(0.3, 0.3, 0.3)]])
    assert jsd(edge, inside, res) == 0.0
    assert jsd(edge[:, :2], inside[:, :2]) == 0.0                # the default 28^3 grid: its last cell begins at 13/28 = 0.464
    assert jsd(edge, inside) > 0                                 # where 0.3 (cell 22) is not in the last cell
    # the default resolution tells 0.3 from 0.35 (cells 22 and 23), resolution 4 does not
    assert jsd(torch.full((1, 1, 3), 0.3), torch.full((1, 1, 3), 0.35)) == 1.0
    assert jsd(torch.full((1, 1, 3), 0.3), torch.full((1, 1, 3), 0.35), res) == 0.0


def test_case_shapes_and_exact_lattices():
    shapes = {"p1": (2, 2, 1), "p2": (2, 2, 2), "p3": (2, 2, 3), "p63": (2, 2, 63), "p64": (2, 2, 64), "p65": (2, 2, 65),
              "p257": (1, 1, 257), "p2048": (1, 1, 2048), "clusters": (1, 1, 256), "permuted": (1, 1, 200), "same_point": (1, 1, 50),
              "two_points": (1, 1, 64), "rect": (3, 5, 33), "union": (7, 7, 96), "lat65": (1, 1, 65), "lat256": (1, 1, 256),
              "lat1d": (1, 1, 100)}
    assert set(shapes) == set(ec.FINITE_CASES + ec.EXACT_CASES)
    for name, (nx, ny, p) in shapes.items():
        x, y = ec.case(name)
        assert x.shape == (nx, p, 3) and y.shape == (ny, p, 3) and x.dtype == torch.float32 and y.dtype == torch.float32, name
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all()), name
    x, y = ec.case("union")
    assert x is y
    for name in ec.EXACT_CASES:
        x, y = ec.case(name)
        for t in (x, y):
            # multiples of 1/8 within [-4, 4.5]: differences m / 8 with |m| <= 68, squares m^2 / 64 and their sums < 2^24 / 64 exact
            assert torch.equal(t * 8, (t * 8).round()) and float(t.abs().max()) <= 4.5, name
        a, b = x[0].numpy(), y[0].numpy()
        s64 = ((a[:, None, :].astype(np.float64) - b[None, :, :].astype(np.float64)) ** 2).sum(axis=2)
        dx, dy, dz = (a[:, None, k] - b[None, :, k] for k in range(3))
        assert np.array_equal((dz * dz + (dy * dy + dx * dx)).astype(np.float64), s64), name
        quantum = ec.quantum_restated(x, y)
        q = ec.quantised(a, b, quantum)
        assert np.array_equal(q, np.rint(np.sqrt(s64).astype(np.float32).astype(np.float64) / quantum).astype(np.int64)), name
        assert len(np.unique(q)) < 0.6 * q.size, name            # many repeated distances (a sum of three squares m^2 / 64 has few values)
    x, y = ec.case("lat1d")
    quantum = ec.quantum_restated(x, y)
    total = ec.emd_quantised(x[0], y[0], quantum)
    assert total * quantum / 100 == 0.5 and ec.emd_float64(x[0], y[0]) == 0.5
    x, y = ec.case("two_points")
    assert len(np.unique(ec.quantised(x[0], y[0], ec.quantum_restated(x, y)))) == 1          # every cost equal
    x, y = ec.case("clusters")
    assert int((x[0, :, 0] > 0.5).sum()) == 128 and int((y[0, :, 0] > 0.5).sum()) == 192


def test_bars_and_default_rounds_are_the_derived_ones():
    assert ec.VALUE_C == 0.75 and ec.VALUE_C >= 0.5 + 3.5 / 16 + 2.0 ** -24 and ec.BITS == 20 and ec.THETA == 4
    assert ec.value_bar(2.0, 2.0 ** -20) == 0.75 * 2.0 ** -20 + 2.0 ** -22
    assert ec.flip_bar(257) == 257
    assert ec.default_max_rounds(2048) == 256 * 2048 + 4096
    text = open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "emd.hip")).read()
    assert re.search(r"EMD_THETA = 4;", text) and re.search(r"EMD_MAX_P = 2048;", text)


@pytest.mark.parametrize("name", ec.FINITE_CASES + ec.EXACT_CASES)
def test_scipy_on_the_integer_matrix_stays_inside_the_value_bar(name):
    """A check of the BAR, not of the kernel (it runs no kernel and passes without one): the exact optimum of the integer matrix
    -- what the kernel is asked to compute, and what tests/test_gpu_emd.py holds it to -- is within VALUE_BAR of the float64 EMD,
    so the bar asks nothing that exact arithmetic on that matrix does not achieve.  Prints the share of the bar used."""
    x, y = ec.case(name)
    quantum = ec.quantum_restated(x, y)
    p = x.shape[1]
    pairs = [(0, 0)] if name == "union" else [(0, y.shape[0] - 1)]
    if name == "union":
        pairs = [(0, 0), (1, 4), (6, 2)]
    if name == "rect":
        pairs = [(0, 0), (2, 4), (1, 3)]
    for i, j in pairs:
        a, b = x[i].numpy(), y[j].numpy()
        e64 = ec.emd_float64(a, b)
        total = ec.emd_quantised(a, b, quantum)
        got = float(ec.out_from_total(total, quantum, p))
        bar = ec.value_bar(e64, quantum)
        used = abs(got - e64) / bar
        print(f"{name}[{i},{j}]: p {p} quantum 2^{int(np.log2(quantum))} emd64 {e64:.9e} integer {total} -> {got:.9e}; uses {used:.3f} of the bar")
        assert abs(got - e64) <= bar, (name, i, j)
        if i == j and name == "union":
            assert total == 0
    if name in ("permuted", "same_point"):
        assert total == 0 and e64 == 0


@pytest.mark.parametrize("name", ("p1", "p2", "p3", "p65", "clusters", "two_points", "same_point", "lat65", "lat1d", "rect"))
def test_auction_restatement_reaches_the_integer_optimum(name):
    """A check of test code only: `auction_restated`, the numpy restatement of the scheme csrc/emd.hip words, reaches scipy's
    optimum on the same integer matrix, so the ROUND COUNTS it prints -- which the default max_rounds rests on -- are those of a
    solver that works.  The kernel itself is held to scipy in tests/test_gpu_emd.py."""
    x, y = ec.case(name)
    quantum = ec.quantum_restated(x, y)
    a, b = x[0].numpy(), y[-1].numpy()
    q = ec.quantised(a, b, quantum)
    total, perm, rounds, bids = ec.auction_restated(q)
    p = q.shape[0]
    print(f"{name}: p {p} rounds {rounds} = {rounds / p:.1f} p, bids {bids}; the default cap is {ec.default_max_rounds(p)}")
    assert sorted(perm.tolist()) == list(range(p))
    assert total == ec.emd_quantised(a, b, quantum) == int(q[np.arange(p), perm].sum())
    assert 4 * rounds <= ec.default_max_rounds(p)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_emd_kernel_uses_no_scratch_and_one_kind_of_atomic(tmp_path):
    csrc = os.path.join(ROOT, "meshdiffusion_amd", "csrc")
    out = tmp_path / "emd.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{ROOT}/include",
                    f"-I{csrc}", os.path.join(csrc, "emd.hip"), "-o", str(out)], check=True, stderr=subprocess.DEVNULL)
    text = out.read_text()
    seen = []
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))      # noqa: E731
        assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
        seen.append(name)
    assert any("md_emd_matrix_kernel" in n for n in seen), seen
    assert "v_mfma" not in text
    # the bid slots' 64-bit LDS maximum, and neither a compare-and-swap loop in its place nor an atomic on global memory
    assert "ds_max_u64" in text and "ds_cmpst" not in text and "global_atomic" not in text and "flat_atomic" not in text
