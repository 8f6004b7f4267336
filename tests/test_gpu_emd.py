"""Earth mover's distance on the GPU (csrc/emd.hip, metrics.emd_matrix) against scipy's linear_sum_assignment: on float64
distances within the derived VALUE_BAR, on the kernel's own integer matrix restated in numpy within FLIP_BAR, and EXACTLY on the
lattice cases (tests/emd_cases.py derives the bars and says why the lattices are exact).  Then the properties the contract
promises -- the same bits from run to run, from either side, from a triangular or a full launch, from a row alone -- the three
ways a pair can fail, and the EMD / JSD figures of `shape_metrics` and tools/eval_shapes.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import emd_cases as ec
import shape_metrics_cases as sm
from conftest import ROOT

pytestmark = pytest.mark.gpu

_REFS = {}


def _ref(name):
    """(x, y, quantum, emd_float64 [Nx,Ny], emd_quantised [Nx,Ny]) of a case, computed once; a union's diagonal and lower half are
    filled from the upper half (the restatements are symmetric)."""
    if name not in _REFS:
        from meshdiffusion_amd.metrics import emd_quantum
        x, y = ec.case(name)
        quantum = emd_quantum(x, y)
        assert quantum == ec.quantum_restated(x, y)
        nx, ny = x.shape[0], y.shape[0]
        e64, tot = np.zeros((nx, ny)), np.zeros((nx, ny), dtype=np.int64)
        for i in range(nx):
            for j in range(ny):
                if y is x and j < i:
                    e64[i, j], tot[i, j] = e64[j, i], tot[j, i]
                elif not (y is x and i == j):
                    e64[i, j], tot[i, j] = ec.emd_float64(x[i], y[j]), ec.emd_quantised(x[i], y[j], quantum)
        _REFS[name] = (x, y, quantum, e64, tot)
    return _REFS[name]


def _run(name, **kw):
    from meshdiffusion_amd.metrics import emd_matrix
    x, y, quantum, e64, tot = _ref(name)
    xg = x.cuda()
    out, info = emd_matrix(xg, xg if y is x else y.cuda(), quantum=quantum, return_info=True, **kw)
    return out, info


def _check_perms(x, y, quantum, info, bar):
    perm, total = info["perm"].cpu().numpy(), info["total"].cpu().numpy()
    p = x.shape[1]
    worst = 0
    for i in range(x.shape[0]):
        for j in range(y.shape[0]):
            assert sorted(perm[i, j].tolist()) == list(range(p)), (i, j)
            q = ec.quantised(x[i].numpy(), y[j].numpy(), quantum)
            cost = int(q[np.arange(p), perm[i, j]].sum())
            worst = max(worst, abs(cost - int(total[i, j])))
            assert abs(cost - int(total[i, j])) <= bar, (i, j, cost, int(total[i, j]))
    return worst


@pytest.mark.parametrize("name", ec.FINITE_CASES)
def test_emd_matrix_against_scipy(hip_lib, name):
    x, y, quantum, e64, tot = _ref(name)
    p = x.shape[1]
    out, info = _run(name)
    got, total, rounds = out.cpu().numpy().astype(np.float64), info["total"].cpu().numpy(), info["rounds"].cpu().numpy()
    bar = ec.value_bar(e64, quantum)
    used = float((np.abs(got - e64) / bar).max())
    flips = int(np.abs(total - tot).max())
    print(f"\n{name}: p {p} pairs {got.size} quantum 2^{int(np.log2(quantum))}; uses {used:.3f} of the value bar; |total - scipy| <= {flips} "
          f"(bar {ec.flip_bar(p)}); rounds min {rounds.min()} median {int(np.median(rounds))} max {rounds.max()} = {rounds.max() / p:.1f} p "
          f"(cap {ec.default_max_rounds(p)})")
    assert out.dtype == torch.float32 and out.shape == (x.shape[0], y.shape[0])
    assert int(info["status"].abs().max()) == 0
    assert bool((np.abs(got - e64) <= bar).all())
    assert flips <= ec.flip_bar(p)
    worst = _check_perms(x, y, quantum, info, ec.flip_bar(p))
    print(f"   cost of perm on the restated integer matrix within {worst} of total")
    assert np.array_equal(out.cpu().numpy(), ec.out_from_total(total, quantum, p))
    again, info2 = _run(name)
    assert torch.equal(again, out) and torch.equal(info2["total"], info["total"])
    if name in ("permuted", "same_point"):
        assert int(total.max()) == 0 and float(out.abs().max()) == 0


@pytest.mark.parametrize("name", ec.EXACT_CASES)
def test_emd_matrix_is_exact_on_lattices(hip_lib, name):
    """Every square and sum is exact in fp32 and both sides round the same square root: a final eps that is too large, a dropped
    phase or a wrong tie rule shows here as total != scipy's."""
    x, y, quantum, e64, tot = _ref(name)
    p = x.shape[1]
    out, info = _run(name)
    total = info["total"].cpu().numpy()
    print(f"\n{name}: p {p} total {total.tolist()} scipy {tot.tolist()} rounds {info['rounds'].tolist()}")
    assert int(info["status"].abs().max()) == 0
    assert np.array_equal(total, tot)
    assert np.array_equal(out.cpu().numpy(), ec.out_from_total(tot, quantum, p))
    assert _check_perms(x, y, quantum, info, 0) == 0
    if name == "lat1d":
        assert float(out[0, 0]) == 0.5


def test_emd_matrix_is_the_same_from_either_side_and_for_a_row_alone(hip_lib):
    from meshdiffusion_amd.metrics import emd_matrix
    x, y, quantum, e64, tot = _ref("rect")
    xg, yg = x.cuda(), y.cuda()
    out = emd_matrix(xg, yg, quantum=quantum)
    assert torch.equal(out, emd_matrix(yg, xg, quantum=quantum).t())
    assert torch.equal(out[1:2], emd_matrix(xg[1:2], yg, quantum=quantum))
    assert torch.equal(out[:, 3:4], emd_matrix(xg, yg[3:4], quantum=quantum))
    # the default quantum is that of the clouds passed
    assert torch.equal(out, emd_matrix(xg, yg))


def test_triangular_launch_equals_the_full_one(hip_lib):
    from meshdiffusion_amd.metrics import emd_matrix
    x, y, quantum, e64, tot = _ref("union")
    xg = x.cuda()
    tri, info = emd_matrix(xg, quantum=quantum, return_info=True)
    full, finfo = emd_matrix(xg, xg.clone(), quantum=quantum, return_info=True)
    n, p = x.shape[0], x.shape[1]
    off = ~torch.eye(n, dtype=torch.bool, device="cuda")
    assert torch.equal(tri[off], full[off]) and torch.equal(info["total"][off], finfo["total"][off])
    assert torch.equal(tri, tri.t()) and torch.equal(info["total"], info["total"].t())
    assert float(tri.diagonal().abs().max()) == 0 and int(info["status"].abs().max()) == 0
    assert int(finfo["total"].diagonal().abs().max()) == 0 and float(full.diagonal().abs().max()) == 0      # a cloud against its copy
    assert torch.equal(emd_matrix(xg, xg, quantum=quantum), tri)                                            # y is x: triangular too
    perm = info["perm"].cpu()
    ident = torch.arange(p, dtype=torch.int32)
    for i in range(n):
        assert torch.equal(perm[i, i], ident)
        for j in range(i + 1, n):                                 # [j][i] holds the inverse of [i][j]
            assert torch.equal(perm[j, i][perm[i, j].long()], ident), (i, j)
    assert int(info["rounds"].diagonal().max()) == 0 and torch.equal(info["rounds"], info["rounds"].t())


def test_a_pair_that_runs_out_of_rounds(hip_lib):
    """A bounded loop ending early: NaN and status 1 for that pair, the others of the launch untouched."""
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.metrics import emd_matrix
    a, b, quantum, e64, tot = _ref("clusters")
    x = a.cuda()
    y = torch.cat([b, a.clone()]).cuda()                           # pair (0, 0): the price war; pair (0, 1): a cloud against its copy
    out, info = emd_matrix(x, y, quantum=quantum, max_rounds=3, return_info=True)
    assert info["status"].tolist() == [[1, 1]] and bool(torch.isnan(out).all())
    assert info["total"].tolist() == [[-1, -1]] and info["rounds"].tolist() == [[3, 3]] and int(info["perm"].max()) == -1
    with pytest.raises(_lib.MeshDiffusionHipError, match=r"pair \(0, 0\).*max_rounds"):
        emd_matrix(x, y, quantum=quantum, max_rounds=3)
    # the triangular launch of (a, b, a) at max_rounds=3: every solved pair is cut short, the diagonal is the exact zero it always is
    tri, tinfo = emd_matrix(torch.cat([a, b, a]).cuda(), quantum=quantum, max_rounds=3, return_info=True)
    assert tinfo["status"].tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]] and float(tri.diagonal().abs().max()) == 0
    assert bool(torch.isnan(tri[~torch.eye(3, dtype=torch.bool, device="cuda")]).all())
    # a cap between the two pairs' needs: a cloud against its copy takes a round or so per phase (the restatement's count is
    # printed, not demanded of the kernel), the price war thousands
    _, _, copy_rounds, _ = ec.auction_restated(ec.quantised(a[0].numpy(), a[0].numpy(), quantum))
    _, _, war_rounds, _ = ec.auction_restated(ec.quantised(a[0].numpy(), b[0].numpy(), quantum))
    cap = 256
    print(f"\nrestated rounds: copy {copy_rounds}, price war {war_rounds}; cap {cap}")
    assert 4 * copy_rounds <= cap and war_rounds >= 4 * cap
    out, info = emd_matrix(x, y, quantum=quantum, max_rounds=cap, return_info=True)
    print(f"kernel rounds {info['rounds'].tolist()}")
    assert info["status"].tolist() == [[1, 0]] and bool(torch.isnan(out[0, 0]))
    assert int(info["total"][0, 1]) == 0 and float(out[0, 1]) == 0.0
    assert sorted(info["perm"][0, 1].tolist()) == list(range(256))
    with pytest.raises(_lib.MeshDiffusionHipError, match=r"pair \(0, 0\).*max_rounds"):
        emd_matrix(x, y, quantum=quantum, max_rounds=cap)
    full, finfo = emd_matrix(x, y, quantum=quantum, return_info=True)
    assert finfo["status"].tolist() == [[0, 0]] and int(finfo["total"][0, 0]) == int(tot[0, 0])


def test_a_quantum_too_small_for_the_data(hip_lib):
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.metrics import emd_matrix
    x, y, quantum, e64, tot = _ref("rect")
    xg, yg = x.cuda(), y.cuda()
    out, info = emd_matrix(xg, yg, quantum=quantum / 1024, return_info=True)      # distances of about 2^28 quanta
    assert bool((info["status"] == 2).all()) and bool(torch.isnan(out).all()) and int(info["rounds"].max()) == 0
    with pytest.raises(_lib.MeshDiffusionHipError, match=r"pair \(0, 0\).*quantum"):
        emd_matrix(xg, yg, quantum=quantum / 1024)
    # two quanta that both suit the data give totals in the ratio of the quanta, up to the rounding of p distances
    coarse, cinfo = emd_matrix(xg, yg, quantum=quantum * 4, return_info=True)
    assert int(cinfo["status"].abs().max()) == 0
    assert int((cinfo["total"] * 4 - torch.as_tensor(tot).cuda()).abs().max()) <= 4 * x.shape[1]


def test_non_finite_coordinates_stay_with_their_cloud(hip_lib):
    from meshdiffusion_amd.metrics import emd_matrix
    x, y, quantum, e64, tot = _ref("rect")
    clean = emd_matrix(x.cuda(), y.cuda(), quantum=quantum)
    for bad in (float("nan"), float("inf"), -float("inf")):
        xb, yb = x.clone(), y.clone()
        xb[1, 4, 1] = bad
        yb[2, 32, 0] = bad
        out, info = emd_matrix(xb.cuda(), yb.cuda(), quantum=quantum, return_info=True)
        want = torch.zeros(3, 5, dtype=torch.int32)
        want[1, :] = 3
        want[:, 2] = 3
        assert torch.equal(info["status"].cpu(), want), bad
        hit = (want == 3).cuda()
        assert bool(torch.isnan(out[hit]).all()) and torch.equal(out[~hit], clean[~hit]), bad
        assert int(info["rounds"][hit].max()) == 0 and int(info["total"][hit].max()) == -1
        # status 3 is not an error, and the default quantum comes from the finite clouds
        plain = emd_matrix(xb.cuda(), yb.cuda())
        assert torch.equal(torch.isnan(plain), hit), bad
    xb = x.clone()
    xb[0, 0, 0] = float("nan")
    tri, info = emd_matrix(xb.cuda(), quantum=quantum, return_info=True)
    assert info["status"].tolist() == [[3, 3, 3], [3, 0, 0], [3, 0, 0]]           # its pair with itself too
    assert bool(torch.isnan(tri[0]).all()) and bool(torch.isnan(tri[1:, 0]).all()) and float(tri[1, 2]) == float(tri[2, 1]) > 0


def test_emd_matrix_refuses_what_it_cannot_do(hip_lib):
    from meshdiffusion_amd import _lib
    from meshdiffusion_amd.metrics import emd_matrix
    x = torch.rand(2, 8, 3, device="cuda")
    with pytest.raises(ValueError, match="same number of points"):
        emd_matrix(x, torch.rand(2, 9, 3, device="cuda"))
    with pytest.raises(ValueError, match="2048"):
        emd_matrix(torch.rand(1, 2049, 3, device="cuda"))
    with pytest.raises(_lib.MeshDiffusionHipError):
        emd_matrix(x, quantum=3.0)
    with pytest.raises(_lib.MeshDiffusionHipError):
        emd_matrix(x, max_rounds=0)
    with pytest.raises(_lib.MeshDiffusionHipError):
        emd_matrix(x.cpu())


# ---- the metrics ------------------------------------------------------------------------------------------------------------
EMD_METRIC_POINTS = 256


@pytest.fixture(scope="module")
def metric_clouds():
    from meshdiffusion_amd.metrics import clouds_from_meshes
    out = {}
    for name in sm.METRIC_CASES:
        s_meshes, r_meshes, us, ur = sm.metric_meshes(name)
        s = clouds_from_meshes(s_meshes, EMD_METRIC_POINTS, uniforms=us[:, :, :EMD_METRIC_POINTS])[0]
        r = s if name == "identical" else clouds_from_meshes(r_meshes, EMD_METRIC_POINTS, uniforms=ur[:, :, :EMD_METRIC_POINTS])[0]
        out[name] = (s, r)
    return out


def _gap_over_bar(d_ss, d_sr, d_rr, quantum):
    """Smallest (second - first) / (bar(first) + bar(second)) over the rows COV uses and the rows 1-NNA uses: above 1, two matrices
    within the value bar of each other have the same argmins."""
    union = torch.cat([torch.cat([d_ss, d_sr], dim=1), torch.cat([d_sr.t(), d_rr], dim=1)], dim=0).clone()
    union.fill_diagonal_(float("inf"))
    worst = float("inf")
    for m in (d_sr, union):
        two = torch.topk(m, 2, dim=1, largest=False).values
        worst = min(worst, float(((two[:, 1] - two[:, 0]) / (ec.value_bar(two[:, 0], quantum) + ec.value_bar(two[:, 1], quantum))).min()))
    return worst


@pytest.mark.parametrize("name", sm.METRIC_CASES)
def test_shape_metrics_with_emd_and_jsd(hip_lib, metric_clouds, name):
    from meshdiffusion_amd import metrics
    s, r = metric_clouds[name]
    S = s.shape[0]
    base = metrics.shape_metrics(s, r.clone())
    got = metrics.shape_metrics(s, r.clone(), emd=True, jsd=True)
    assert set(got) == set(base) | {"mmd_emd", "cov_emd", "1nna_emd", "1nna_emd_sample", "1nna_emd_ref", "emd_quantum", "jsd"}
    for k, v in base.items():
        assert got[k] == v, k
    assert set(metrics.shape_metrics(s, r.clone(), jsd=True)) == set(base) | {"jsd"}
    quantum = metrics.emd_quantum(s, r)
    assert got["emd_quantum"] == quantum == ec.quantum_restated(s.cpu(), r.cpu())
    e = ec.emd_float64_matrix(torch.cat([s, r]).cpu().numpy(), torch.cat([s, r]).cpu().numpy())
    e = torch.minimum(e, e.t())                                    # scipy's two orders of a pair agree to the last bits only
    d_ss, d_sr, d_rr = e[:S, :S], e[:S, S:], e[S:, S:]
    gap = _gap_over_bar(d_ss, d_sr, d_rr, quantum)
    mmd, cov = sm.mmd_cov_restated(d_sr)
    nna = sm.one_nna_restated(d_ss, d_sr, d_rr)
    print(f"\n{name}: {got}\n   float64: mmd {mmd:.9e} cov {cov} 1-nna {nna}; smallest argmin gap {gap:.1f} bars")
    assert gap > 1                                                 # the input condition, on the clouds sampled here
    assert got["cov_emd"] == cov and (got["1nna_emd"], got["1nna_emd_sample"], got["1nna_emd_ref"]) == nna
    assert abs(got["mmd_emd"] - mmd) <= ec.value_bar(float(d_sr.max()), quantum)
    assert got["jsd"] == metrics.jsd(s, r) and abs(got["jsd"] - metrics.jsd(s.cpu(), r.cpu())) < 1e-12 and 0 <= got["jsd"] <= 1
    if name == "identical":
        assert got["mmd_emd"] == 0 and got["cov_emd"] == 1 and got["1nna_emd"] == 0 and got["jsd"] == 0
    if name == "families":
        assert got["1nna_emd"] == 1 and got["jsd"] > 0.5
    with pytest.raises(ValueError, match="same number of points"):
        metrics.shape_metrics(s, r[:, :200], emd=True)


def test_eval_shapes_tool_prints_the_emd_and_jsd_figures(hip_lib, tmp_path):
    from meshdiffusion_amd import mesh_export
    from meshdiffusion_amd.metrics import clouds_from_meshes, normalize_clouds, shape_metrics
    meshes = {"samples": [sm.sphere_mesh(0.3), sm.torus_mesh(0.4, 0.1, 0.0)], "ref": [sm.sphere_mesh(0.35), sm.torus_mesh(0.5, 0.1, 1.0)]}
    for d, ms in meshes.items():
        os.makedirs(tmp_path / d)
        for k, (v, f) in enumerate(ms):
            mesh_export.save_obj(str(tmp_path / d / f"{k:06d}.obj"), v, f, decimal_places=8)
    out_json = tmp_path / "metrics.json"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_shapes.py"), "--samples", str(tmp_path / "samples"), "--ref",
                          str(tmp_path / "ref"), "--points", "512", "--seed", "11", "--emd", "--jsd", "--out", str(out_json)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    assert rec == json.load(open(out_json))
    gen = torch.Generator(device="cuda").manual_seed(11)
    loaded = {d: [mesh_export.load_obj(str(tmp_path / d / f"{k:06d}.obj")) for k in range(2)] for d in meshes}
    s = clouds_from_meshes(loaded["samples"], 512, generator=gen)[0]
    r = clouds_from_meshes(loaded["ref"], 512, generator=gen)[0]
    want = shape_metrics(normalize_clouds(s, "bbox"), normalize_clouds(r, "bbox"), emd=True, jsd=True)
    print(f"\neval_shapes.py --emd --jsd: {rec}")
    assert {"mmd_emd", "cov_emd", "1nna_emd", "emd_quantum", "jsd"} <= set(want)
    for k, v in want.items():
        assert rec[k] == v, k
    assert rec["skipped_sample"] == 0 and rec["skipped_ref"] == 0 and rec["seconds"] > 0
