"""The CSR of every gather of the fitting stack, host side (no GPU): `csr_by_row` against a Python-loop restatement, and the row
loop of csrc/md_gather.h as a stand-alone host program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _csr_loop(dest, n_rows):
    """(ptr, order) of a 1-D table as Python lists: the codes of row 0 in ascending order, then those of row 1, ..."""
    dest = [int(d) for d in dest]
    ptr, order = [0], []
    for r in range(n_rows):
        order += [k for k, d in enumerate(dest) if d == r]
        ptr.append(len(order))
    return ptr, order


CASES = {                                                            # name: (dest, n_rows)
    "no_codes": ([], 5),
    "one_row": ([0, 0, 0], 1),
    "one_row_no_codes": ([], 1),
    "empty_rows_at_start_middle_end": ([2, 1, 5, 2, 1, 5], 8),       # rows 0, 3, 4, 6, 7 have no codes
    "all_codes_in_one_row": ([3] * 7, 6),
    "repeated_destinations": ([4, 0, 4, 4, 1, 0, 4, 1, 0, 4], 5),    # stable: ascending position inside a row
    "descending": (list(range(9, -1, -1)), 10),
}


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("name", list(CASES))
def test_csr_by_row_equals_the_loop(name, dtype):
    from meshdiffusion_amd._csr import csr_by_row
    dest, n_rows = CASES[name]
    ptr, order = csr_by_row(torch.tensor(dest, dtype=dtype), n_rows)
    want_ptr, want_order = _csr_loop(dest, n_rows)
    assert ptr.dtype == torch.int32 and order.dtype == torch.int32
    assert ptr.is_contiguous() and order.is_contiguous()
    assert ptr.shape == (n_rows + 1,) and order.shape == (len(dest),)
    assert ptr.tolist() == want_ptr and order.tolist() == want_order


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_csr_by_row_batched_rows_have_their_own_tables(dtype):
    from meshdiffusion_amd._csr import csr_by_row
    n_rows = 6
    table = [[5, 0, 5, 2, 2, 0, 5], [1, 1, 1, 1, 1, 1, 1]]           # B = 2: a spread table and one with every code in row 1
    ptr, order = csr_by_row(torch.tensor(table, dtype=dtype), n_rows)
    assert ptr.dtype == torch.int32 and order.dtype == torch.int32
    assert ptr.is_contiguous() and order.is_contiguous()
    assert ptr.shape == (2, n_rows + 1) and order.shape == (2, 7)
    for b in range(2):
        want_ptr, want_order = _csr_loop(table[b], n_rows)
        assert ptr[b].tolist() == want_ptr and order[b].tolist() == want_order
    ptr0, order0 = csr_by_row(torch.zeros((2, 0), dtype=dtype), n_rows)         # B = 2, K = 0
    assert ptr0.dtype == order0.dtype == torch.int32 and ptr0.tolist() == [[0] * (n_rows + 1)] * 2 and order0.shape == (2, 0)
    # a transposed (non-contiguous) table gives the bits of its contiguous copy
    t = torch.tensor(table, dtype=dtype).t().contiguous().t()
    assert not t.is_contiguous()
    ptr_t, order_t = csr_by_row(t, n_rows)
    assert torch.equal(ptr_t, ptr) and torch.equal(order_t, order) and ptr_t.is_contiguous() and order_t.is_contiguous()


def test_csr_by_row_refuses_what_does_not_fit_int32():
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd._csr import csr_by_row
    with pytest.raises(_lib.MeshDiffusionHipError, match="MD_ERR_UNSUPPORTED"):
        csr_by_row(torch.zeros(3, dtype=torch.int64), 2 ** 31 - 1)              # ptr would need n_rows + 1 > int32 max values
    with pytest.raises(_lib.MeshDiffusionHipError, match="MD_ERR_UNSUPPORTED"):
        csr_by_row(torch.zeros(1, dtype=torch.int8).expand(2 ** 31), 4)         # K = 2^31 codes (a stride-0 view: no memory)


def test_the_named_callers_are_csr_by_row():
    from meshdiffusion_amd import dmtet, pointcloud
    from meshdiffusion_amd._csr import csr_by_row
    faces = torch.tensor([[0, 1, 2], [2, 1, 3], [0, 2, 3]])
    for got, want in ((dmtet.face_corner_csr(faces, 5), csr_by_row(faces.reshape(-1), 5)),
                      (pointcloud._csr(faces.t().contiguous(), 4), csr_by_row(faces.t().contiguous(), 4))):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_gather_row_host_program_under_sanitizers(tmp_path):
    """tests/host/gather_row_main.hip: md_gather_row<W, KAHAN> on host arrays for W in {1, 3, 8} and both sum kinds, an empty
    row, the four guards on a broken CSR, and the sequences that separate a plain from a compensated sum.  Built host-only with
    the address and undefined-behaviour sanitizers on the host compilation alone (no kernel is instantiated, nothing is built
    for or run on a GPU) and run as a child process of its own."""
    exe = tmp_path / "gather_row_main"
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                    f"-I{ROOT}/include", f"-I{ROOT}/meshdiffusion_amd/csrc", os.path.join(ROOT, "tests", "host", "gather_row_main.hip"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "gather_row: ok" in res.stdout and "runtime error" not in res.stderr, res.stdout + res.stderr
