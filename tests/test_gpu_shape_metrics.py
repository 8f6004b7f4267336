"""Generation metrics on the GPU: md_sided_mean_matrix and meshdiffusion_amd/metrics.py against the float64 restatements of
tests/shape_metrics_cases.py (which run on the GPU too, in torch float64).

Bars, none fitted to what the kernel gives (derivations in shape_metrics_cases.py):
  sided matrix          |out - out64| <= 1.125 * 2^-20 * out64 for EVERY entry of every finite case; `lattice` bit for bit
  chamfer_matrix        against pointcloud.chamfer_distance pair by pair: relative difference <= 2^-23 (the same fp32 minima,
                        float64 sums in another order, one fp32 rounding)
  COV, 1-NNA            equal to the float64 restatement exactly, on sets whose argmins are separated by more than 2^-18
                        (tests/test_cpu_shape_metrics_host.py; re-checked here on the sampled clouds)
Each test prints its figures before it asserts.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import shape_metrics_cases as sm
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _case(name):
    x, y = sm.case(name)
    xc = x.cuda()
    return xc, (xc if y is x else y.cuda())


@pytest.mark.parametrize("name", sm.FINITE_CASES)
def test_sided_mean_matrix_against_float64(hip_lib, name):
    from meshdiffusion_amd.metrics import sided_mean_matrix
    x, y = _case(name)
    out = sided_mean_matrix(x, y)
    assert out.dtype == torch.float32 and out.shape == (x.shape[0], y.shape[0])
    out64 = sm.sided_mean_float64(x, y)
    ok, worst = sm.within_bar(out, out64)
    print(f"\n{name}: {tuple(out.shape)} entries, worst |out - out64| / out64 {worst:.3e} (bar {sm.VALUE_BAR:.3e})")
    assert ok, name
    assert torch.equal(out, sided_mean_matrix(x, y))                         # bit-identical from run to run
    if name == "lattice":
        assert out.tolist() == sm.LATTICE_EXPECTED
    if name == "self":
        assert not bool(torch.diagonal(out).any())


def test_self_chamfer_matrix_is_symmetric_with_a_zero_diagonal(hip_lib):
    from meshdiffusion_amd.metrics import chamfer_matrix
    x, _ = _case("self")
    d = chamfer_matrix(x)
    assert d.shape == (9, 9) and torch.equal(d, d.t()) and not bool(torch.diagonal(d).any())
    assert torch.equal(d, chamfer_matrix(x, x)) and torch.equal(d, chamfer_matrix(x, x.clone()))
    ok, worst = sm.within_bar(d, sm.chamfer_float64(x), sm.VALUE_BAR + 2.0 ** -24)
    print(f"\nself: chamfer matrix worst relative error {worst:.3e}")
    assert ok and float(d[0, 1]) > 0


def test_result_does_not_depend_on_the_run_length(hip_lib):
    """Rows computed one y cloud at a time (ny = 1: a run of one) equal the rows of the whole launch bit for bit."""
    from meshdiffusion_amd.metrics import sided_mean_matrix
    for name in ("runs", "run3", "run_tail"):
        x, y = _case(name)
        xs = x[:8]
        whole = sided_mean_matrix(x, y)[:8]
        single = torch.cat([sided_mean_matrix(xs, y[j:j + 1]) for j in range(y.shape[0])], dim=1)
        assert torch.equal(whole, single), name
        assert torch.equal(whole[:1], sided_mean_matrix(x[:1], y)), name     # and not on nx either


def test_chamfer_matrix_agrees_with_chamfer_distance(hip_lib):
    from meshdiffusion_amd.metrics import chamfer_matrix
    from meshdiffusion_amd.pointcloud import chamfer_distance
    x, y = _case("typical")
    d = chamfer_matrix(x, y)
    nx, ny = d.shape
    pairs = chamfer_distance(x[:, None].expand(-1, ny, -1, -1).reshape(nx * ny, -1, 3),
                             y[None].expand(nx, -1, -1, -1).reshape(nx * ny, -1, 3)).reshape(nx, ny)
    one = chamfer_distance(x[2:3], y[5:6])
    rel = ((d.double() - pairs.double()).abs() / pairs.double()).max()
    print(f"\ntypical: worst relative difference from chamfer_distance {float(rel):.3e} (bar {sm.CONSISTENCY_BAR:.3e})")
    assert float(one[0]) == float(pairs[2, 5])
    assert float(rel) <= sm.CONSISTENCY_BAR


def test_non_finite_coordinates(hip_lib):
    from meshdiffusion_amd.metrics import sided_mean_matrix
    x, y, clean_x, clean_y = sm.nonfinite_case()
    x, y = x.cuda(), y.cuda()
    out = sided_mean_matrix(x, y)
    want = sm.sided_mean_fp32(x, y)
    print(f"\nnonfinite: NaN entries {int(torch.isnan(out).sum())} (torch {int(torch.isnan(want).sum())}), infinite "
          f"{int(torch.isinf(out).sum())} (torch {int(torch.isinf(want).sum())})")
    assert torch.equal(torch.isnan(out), torch.isnan(want)) and torch.equal(torch.isinf(out), torch.isinf(want))
    assert int(torch.isnan(out).sum()) > 0 and int(torch.isinf(out).sum()) > 0
    fin = torch.isfinite(want)
    out64 = sm.sided_mean_float64(x, y)
    assert bool(((out.double() - out64).abs()[fin] <= sm.VALUE_BAR * out64[fin]).all())
    tx, ty = _case("tiny")
    clean = sided_mean_matrix(tx, ty)
    ix, iy = torch.tensor(clean_x, device="cuda"), torch.tensor(clean_y, device="cuda")
    assert torch.equal(out[ix][:, iy], clean[ix][:, iy])                      # the careful loop gives the fast loop's bits
    # the other direction, where the non-finite cloud is the resident block
    back, want_back = sided_mean_matrix(y, x), sm.sided_mean_fp32(y, x)
    assert torch.equal(torch.isnan(back), torch.isnan(want_back)) and torch.equal(torch.isinf(back), torch.isinf(want_back))
    assert torch.equal(back[iy][:, ix], sided_mean_matrix(ty, tx)[iy][:, ix])


@pytest.mark.parametrize("name", sm.NONFINITE_TILE_CASES)
def test_non_finite_point_outside_the_last_tile(hip_lib, name):
    """A NaN met in an early tile of a y cloud survives the finite tiles after it, in both directions, as in torch."""
    from meshdiffusion_amd.metrics import sided_mean_matrix
    x, y, clean = (t.cuda() for t in sm.nonfinite_tile_case(name))
    for a, b, b_clean in ((x, y, clean), (y, x, x)):
        out, want = sided_mean_matrix(a, b), sm.sided_mean_fp32(a, b)
        print(f"\n{name} {tuple(out.shape)}: NaN {torch.isnan(out).tolist()} torch {torch.isnan(want).tolist()}")
        assert torch.equal(torch.isnan(out), torch.isnan(want)) and torch.equal(torch.isinf(out), torch.isinf(want))
        assert int(torch.isnan(out).sum()) == 2                               # y[0] against both x clouds, whichever side it is on
        fin = torch.isfinite(want)
        out64 = sm.sided_mean_float64(a, b)
        assert bool(((out.double() - out64).abs()[fin] <= sm.VALUE_BAR * out64[fin]).all())
        was = sided_mean_matrix(clean if a is y else a, b_clean)
        assert torch.equal(out[fin], was[fin])                                # the untouched pairs keep the fast loop's bits


def test_cpu_tensors_and_wrong_ranks_raise(hip_lib):
    from meshdiffusion_amd import _lib, metrics
    x = torch.rand(2, 5, 3)
    with pytest.raises(_lib.MeshDiffusionHipError):
        metrics.sided_mean_matrix(x, x.cuda())
    with pytest.raises(_lib.MeshDiffusionHipError):
        metrics.chamfer_matrix(x.cuda(), x)
    for bad in (torch.rand(5, 3), torch.rand(2, 5, 2), torch.rand(2, 0, 3), torch.rand(1, 2, 5, 3)):
        with pytest.raises(ValueError):
            metrics.sided_mean_matrix(bad.cuda(), x.cuda())
        with pytest.raises(ValueError):
            metrics.chamfer_matrix(x.cuda(), bad.cuda())


@pytest.fixture(scope="module")
def metric_clouds():
    from meshdiffusion_amd.metrics import clouds_from_meshes
    out = {}
    for name in sm.METRIC_CASES:
        s_meshes, r_meshes, us, ur = sm.metric_meshes(name)
        s, skipped = clouds_from_meshes(s_meshes, sm.METRIC_POINTS, uniforms=us)
        assert skipped == [] and s.shape == (6, sm.METRIC_POINTS, 3) and s.is_cuda
        r = s if name == "identical" else clouds_from_meshes(r_meshes, sm.METRIC_POINTS, uniforms=ur)[0]
        out[name] = (s, r)
    return out


def _restated(s, r):
    """(mmd, cov, (1-nna overall, samples, references), smallest argmin gap) in float64 on the clouds given."""
    d_ss, d_sr, d_rr = sm.chamfer_float64(s), sm.chamfer_float64(s, r), sm.chamfer_float64(r)
    return sm.mmd_cov_restated(d_sr) + (sm.one_nna_restated(d_ss, d_sr, d_rr), sm.argmin_gaps(d_ss, d_sr, d_rr),)


@pytest.mark.parametrize("name", sm.METRIC_CASES)
def test_shape_metrics_on_constructed_sets(hip_lib, metric_clouds, name):
    from meshdiffusion_amd.metrics import shape_metrics
    s, r = metric_clouds[name]
    got = shape_metrics(s, r.clone())
    mmd, cov, nna, gap = _restated(s, r)
    print(f"\n{name}: {got}\n   float64: mmd {mmd:.9e} cov {cov} 1-nna {nna}; smallest argmin gap {gap:.3e}")
    assert gap > sm.ARGMIN_GAP                                               # the input condition, on the clouds sampled here
    assert set(got) == {"mmd_cd", "cov_cd", "1nna_cd", "1nna_cd_sample", "1nna_cd_ref", "n_sample", "n_ref", "points"}
    assert (got["n_sample"], got["n_ref"], got["points"]) == (6, 6, [sm.METRIC_POINTS, sm.METRIC_POINTS])
    assert got["cov_cd"] == cov and (got["1nna_cd"], got["1nna_cd_sample"], got["1nna_cd_ref"]) == nna
    assert abs(got["mmd_cd"] - mmd) <= (sm.VALUE_BAR + 2.0 ** -24) * mmd
    if name == "identical":
        assert got["mmd_cd"] == 0 and got["cov_cd"] == 1 and got["1nna_cd"] == 0
    if name == "families":
        assert got["1nna_cd"] == 1


def test_shape_metrics_with_unequal_point_counts_and_a_nan(hip_lib, metric_clouds):
    from meshdiffusion_amd.metrics import shape_metrics
    s, r = metric_clouds["concentric"]
    fewer = shape_metrics(s, r[:, :1500])                                    # P != Q: three chamfer matrices
    mmd, cov, nna, gap = _restated(s, r[:, :1500])
    print(f"\nunequal: {fewer}\n   float64: mmd {mmd:.9e} cov {cov} 1-nna {nna}; smallest argmin gap {gap:.3e}")
    assert gap > sm.ARGMIN_GAP and fewer["points"] == [sm.METRIC_POINTS, 1500]
    assert fewer["cov_cd"] == cov and (fewer["1nna_cd"], fewer["1nna_cd_sample"], fewer["1nna_cd_ref"]) == nna
    assert abs(fewer["mmd_cd"] - mmd) <= (sm.VALUE_BAR + 2.0 ** -24) * mmd
    bad = r.clone()
    bad[4, 17, 2] = float("nan")
    with pytest.raises(ValueError, match="reference cloud 4"):
        shape_metrics(s, bad)
    bad = s.clone()
    bad[2, 0, 0] = float("inf")
    with pytest.raises(ValueError, match="sample cloud 2"):
        shape_metrics(bad, r[:, :1500])


def test_clouds_from_meshes_empty_meshes(hip_lib):
    from meshdiffusion_amd.metrics import clouds_from_meshes
    v, f = sm.sphere_mesh(0.3)
    empty = (v, torch.zeros(0, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="mesh 1 "):
        clouds_from_meshes([(v, f), empty], 64)
    u = torch.rand(3, 3, 64, generator=torch.Generator().manual_seed(1))
    clouds, skipped = clouds_from_meshes([(v, f), empty, (v.numpy() * 2, f.numpy())], 64, uniforms=u, skip_empty=True)
    assert skipped == [1] and clouds.shape == (2, 64, 3)
    alone, _ = clouds_from_meshes([(v * 2, f)], 64, uniforms=u[:, 2:3])      # mesh k draws uniforms[:, k]
    assert torch.equal(clouds[1], alone[0])


def test_eval_shapes_tool_prints_the_api_figures(hip_lib, tmp_path):
    from meshdiffusion_amd import mesh_export
    from meshdiffusion_amd.metrics import clouds_from_meshes, normalize_clouds, shape_metrics
    meshes = {"samples": [sm.sphere_mesh(0.3), sm.torus_mesh(0.4, 0.1, 0.0)], "ref": [sm.sphere_mesh(0.35), sm.torus_mesh(0.5, 0.1, 1.0)]}
    for d, ms in meshes.items():
        os.makedirs(tmp_path / d)
        for k, (v, f) in enumerate(ms):
            mesh_export.save_obj(str(tmp_path / d / f"{k:06d}.obj"), v, f, decimal_places=8)
    out_json = tmp_path / "metrics.json"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_shapes.py"), "--samples", str(tmp_path / "samples"), "--ref",
                          str(tmp_path / "ref"), "--points", "512", "--seed", "11", "--out", str(out_json)], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    assert rec == json.load(open(out_json))
    gen = torch.Generator(device="cuda").manual_seed(11)
    loaded = {d: [mesh_export.load_obj(str(tmp_path / d / f"{k:06d}.obj")) for k in range(2)] for d in meshes}
    s = clouds_from_meshes(loaded["samples"], 512, generator=gen)[0]
    r = clouds_from_meshes(loaded["ref"], 512, generator=gen)[0]
    want = shape_metrics(normalize_clouds(s, "bbox"), normalize_clouds(r, "bbox"))
    print(f"\neval_shapes.py: {rec}")
    for k, v in want.items():
        assert rec[k] == v, k
    assert rec["skipped_sample"] == 0 and rec["skipped_ref"] == 0 and rec["seconds"] > 0
