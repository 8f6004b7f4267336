"""The light-field distance on the GPU (csrc/lfd.hip, meshdiffusion_amd/lfd.py) against the float64 restatement of its contract
(tests/lfd_cases.py): the descriptor's coefficients within the derived DESC_BAR, its bytes equal wherever float64 is clear of a
rounding boundary, the matrix EQUAL to the integer loops, and the properties the contract promises -- the same bits from run to
run, from a triangular or a full launch, from a row alone.  Then three small meshes end to end."""
import numpy as np
import pytest
import torch

import lfd_cases as lc
import shape_metrics_cases as sm

pytestmark = pytest.mark.gpu

_BY_RES = {}
for _name in lc.GPU_CASES:
    _BY_RES.setdefault(lc.CASES[_name].shape[0], []).append(_name)


def _describe(names):
    from meshdiffusion_amd import lfd
    masks = torch.from_numpy(np.stack([lc.CASES[k] for k in names])).cuda()
    desc, coef, status = lfd.describe(masks, return_info=True)
    again = lfd.describe(masks, return_info=True)
    assert all(torch.equal(a, b) for a, b in zip((desc, coef, status), again))              # two runs: the same bits
    assert torch.equal(lfd.describe(masks), desc) and torch.equal(lfd.describe(masks.bool()), desc)
    return desc.cpu().numpy(), coef.cpu().numpy().astype(np.float64), status.cpu().numpy()


@pytest.mark.parametrize("R", sorted(_BY_RES))
def test_descriptor_against_float64(hip_lib, R):
    """One launch per resolution with every case of it: more masks than one workgroup takes (it takes one)."""
    names = _BY_RES[R]
    assert R in (16, 33, 64, 256) and (len(names) > 1 or R == 256)
    desc, coef, status = _describe(names)
    assert desc.shape == (len(names), 48) and desc.dtype == np.uint8 and coef.shape == (len(names), 45)
    for k, name in enumerate(names):
        c64, b64, s64 = lc.reference(name)
        share = np.abs(coef[k] - c64) / lc.COEF_BAR
        clear = ~lc.near_half(c64)
        print(f"\n{name}: uses {share.max():.3f} of the bar (value {int(share.argmax())}); {int((desc[k] != b64).sum())} bytes differ, "
              f"{int(clear.sum())} of 45 must be equal")
        assert status[k] == s64
        assert not desc[k, 45:].any()
        assert bool((share <= 1).all()), (name, int(share.argmax()), float(share.max()))
        assert int(np.abs(desc[k].astype(np.int64) - b64.astype(np.int64)).max()) <= 1
        assert np.array_equal(desc[k, :45][clear], b64[:45][clear])
        if s64 == 1:
            assert not desc[k].any() and not coef[k].any()


def test_descriptor_of_one_mask_does_not_depend_on_its_batch(hip_lib):
    from meshdiffusion_amd import lfd
    names = _BY_RES[33]
    masks = torch.from_numpy(np.stack([lc.CASES[k] for k in names])).cuda()
    desc, coef, _ = lfd.describe(masks, return_info=True)
    for k in (0, len(names) - 1):
        d1, c1, _ = lfd.describe(masks[k:k + 1].clone(), return_info=True)
        assert torch.equal(d1[0], desc[k]) and torch.equal(c1[0], coef[k])
    with pytest.raises(Exception):
        lfd.describe(torch.zeros((1, 513, 513), dtype=torch.uint8, device="cuda"))


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------
def _perm(G):
    from meshdiffusion_amd import lfd
    return lfd.rotation_perms()[:G] if G <= 60 else None


@pytest.mark.parametrize("nx,ny,L,G", [(1, 1, 1, 1), (3, 5, 2, 60), (2, 9, 3, 60), (17, 17, 10, 60)])
def test_matrix_equals_numpy(hip_lib, nx, ny, L, G):
    """(2, 9, ...): one y model past the run a workgroup owns (MD_LFD_RUN = 8).  (17, 17, 10, 60): x against itself, full and
    triangular."""
    from meshdiffusion_amd import lfd
    assert lfd.RUN == 8
    perm = _perm(G)
    x = lc.random_models(nx, L, 100 + nx)
    y = x if (nx, ny) == (17, 17) else lc.random_models(ny, L, 200 + ny)
    want = lc.matrix_numpy(x, y, perm)
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    full = lfd.lfd_matrix(xg, yg.clone(), perms=perm)
    assert full.dtype == torch.int32 and np.array_equal(full.cpu().numpy(), want)
    assert torch.equal(lfd.lfd_matrix(xg, yg.clone(), perms=perm), full)
    for j in (0, ny - 1):                                                                   # a row alone: one y model at a time
        assert torch.equal(lfd.lfd_matrix(xg, yg[j:j + 1].clone(), perms=perm)[:, 0], full[:, j])
    if y is x:
        tri = lfd.lfd_matrix(xg, perms=perm)
        assert torch.equal(tri, full) and torch.equal(tri, tri.t()) and not bool(tri.diagonal().any())
        assert torch.equal(lfd.lfd_matrix(xg, xg, perms=perm), tri)


def test_matrix_extremes_and_a_known_match(hip_lib):
    from meshdiffusion_amd import lfd
    perms = lfd.rotation_perms()
    zeros = torch.zeros((2, 10, 10, 48), dtype=torch.uint8, device="cuda")
    ones = torch.full((3, 10, 10, 48), 255, dtype=torch.uint8, device="cuda")
    assert bool((lfd.lfd_matrix(zeros, ones) == 122400).all()) and bool((lfd.lfd_matrix(ones, zeros) == 122400).all())
    # y[j] is x[j] with its light fields swapped and its views carried along by rotation g: exactly 0 on the diagonal, and
    # (random bytes) nowhere else
    x = lc.random_models(4, 10, 7)
    y = np.zeros_like(x)
    swap = np.roll(np.arange(10), 3)
    for j in range(4):
        g = (11, 0, 37, 59)[j]
        for lb in range(10):
            y[j, lb, perms[g]] = x[j, swap[lb]]                                             # y[lb][perm[g][v]] = x[swap[lb]][v]
    out = lfd.lfd_matrix(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()).cpu().numpy()
    assert np.array_equal(out, lc.matrix_numpy(x, y, perms))
    assert not out.diagonal().any() and bool((out[~np.eye(4, dtype=bool)] > 0).all())


def test_matrix_refuses_what_the_contract_refuses(hip_lib):
    from meshdiffusion_amd import lfd
    x = torch.zeros((2, 2, 10, 48), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="perms"):
        lfd.lfd_matrix(x, perms=np.full((1, 10), 10))
    with pytest.raises(ValueError):
        lfd.lfd_matrix(x, torch.zeros((2, 3, 10, 48), dtype=torch.uint8, device="cuda"))
    with pytest.raises(Exception):
        lfd.lfd_matrix(x.cpu())


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _as_gpu(mesh):
    v, f = mesh
    return torch.as_tensor(np.asarray(v), dtype=torch.float32).cuda(), torch.as_tensor(np.asarray(f)).to(torch.int64).cuda()


def test_three_meshes_end_to_end(hip_lib):
    from meshdiffusion_amd import lfd
    box_v, box_f = lc.box_mesh(1.0, 2.0, 3.0)
    g = lfd.rotation_matrices()[23]
    assert not np.allclose(g, np.eye(3))
    meshes = [sm.sphere_mesh(0.5), sm.torus_mesh(0.4, 0.12, 0.0), (box_v, box_f), (box_v @ g.T, box_f), sm.sphere_mesh(0.3),
              sm.torus_mesh(0.35, 0.15, 0.0)]
    sil = lfd.silhouettes(*_as_gpu(meshes[2]), resolution=64, L=10)
    assert sil.shape == (100, 64, 64) and sil.dtype == torch.uint8 and int(sil.max()) == 1
    assert int(sil.reshape(100, -1).sum(dim=1).min()) > 0                                   # every view sees the box
    desc, skipped = lfd.lfd_descriptors([_as_gpu(m) for m in meshes], resolution=64, L=10)
    assert desc.shape == (6, 10, 10, 48) and desc.dtype == torch.uint8 and skipped == []
    d = lfd.lfd_matrix(desc)
    dn = d.cpu().numpy()
    print(f"\nLFD at 64^2: box to turned box {dn[2, 3]}, box to torus {dn[2, 1]}, box to sphere {dn[2, 0]}, sphere to torus {dn[0, 1]}, "
          f"sphere to smaller sphere {dn[0, 4]}; turned box / torus = {dn[2, 3] / dn[2, 1]:.3f}")
    assert np.array_equal(dn, lc.matrix_numpy(desc.cpu().numpy(), desc.cpu().numpy(), lfd.rotation_perms()))
    assert np.array_equal(dn, dn.T) and not dn.diagonal().any()
    assert dn[2, 3] < dn[2, 1] and dn[2, 3] < dn[2, 0]
    # samples: sphere, torus, box; references: turned box, smaller sphere, fatter torus
    rec = lfd.lfd_metrics(desc[:3], desc[3:])
    d64 = d.to(torch.float64).cpu()
    mmd, cov = sm.mmd_cov_restated(d64[:3, 3:])
    acc = sm.one_nna_restated(d64[:3, :3], d64[:3, 3:], d64[3:, 3:])
    assert rec["mmd_lfd"] == pytest.approx(mmd, rel=1e-12) and rec["cov_lfd"] == cov
    assert (rec["1nna_lfd"], rec["1nna_lfd_sample"], rec["1nna_lfd_ref"]) == pytest.approx(acc, rel=1e-12)
    assert rec["n_sample"] == 3 and rec["n_ref"] == 3
    # a mesh without faces is named, or skipped
    empty = (torch.zeros((3, 3)), torch.zeros((0, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="mesh 1"):
        lfd.lfd_descriptors([_as_gpu(meshes[0]), empty], resolution=64, L=2)
    two, skipped = lfd.lfd_descriptors([_as_gpu(meshes[0]), empty], resolution=64, L=2, skip_empty=True)
    assert two.shape == (1, 2, 10, 48) and skipped == [1]


def test_eval_shapes_tool_adds_the_lfd_figures(hip_lib, tmp_path, capsys):
    """tools/eval_shapes.py --lfd, in this process: its figures are those of the API on the meshes it loads, and without the flag
    the record has no LFD key."""
    import importlib.util
    import json
    import os
    from conftest import ROOT
    from meshdiffusion_amd import lfd, mesh_export
    meshes = {"samples": [sm.sphere_mesh(0.3), sm.torus_mesh(0.4, 0.1, 0.0)], "ref": [sm.sphere_mesh(0.35), lc.box_mesh(1.0, 2.0, 3.0)]}
    for d, ms in meshes.items():
        os.makedirs(tmp_path / d)
        for k, (v, f) in enumerate(ms):
            mesh_export.save_obj(str(tmp_path / d / f"{k:06d}.obj"), torch.as_tensor(np.asarray(v), dtype=torch.float32),
                                 torch.as_tensor(np.asarray(f)), decimal_places=8)
    spec = importlib.util.spec_from_file_location("eval_shapes_tool", os.path.join(ROOT, "tools", "eval_shapes.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    argv = ["--samples", str(tmp_path / "samples"), "--ref", str(tmp_path / "ref"), "--points", "256"]
    tool.main(argv)
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not any("lfd" in k for k in plain)
    tool.main(argv + ["--lfd", "--lfd_res", "64", "--lfd_fields", "3"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    loaded = {d: [mesh_export.load_obj(str(tmp_path / d / f"{k:06d}.obj")) for k in range(2)] for d in meshes}
    want = lfd.lfd_metrics(lfd.lfd_descriptors(loaded["samples"], 64, 3)[0], lfd.lfd_descriptors(loaded["ref"], 64, 3)[0])
    for k in ("mmd_lfd", "cov_lfd", "1nna_lfd", "1nna_lfd_sample", "1nna_lfd_ref"):
        assert rec[k] == want[k], k
    assert (rec["lfd_res"], rec["lfd_fields"], rec["skipped_sample_lfd"], rec["skipped_ref_lfd"]) == (64, 3, 0, 0)
    assert {k: v for k, v in rec.items() if "lfd" not in k and k != "seconds"} == {k: v for k, v in plain.items() if k != "seconds"}
