"""The host side of the light-field distance (meshdiffusion_amd/lfd.py) and the conditions under which tests/test_gpu_lfd.py may
ask what it asks: the rotation table is the rotation group of the dodecahedron, the light fields are apart, the fp32 scheme of
the contract stays inside DESC_BAR of float64 on every case, no case has a pixel at a bin boundary or too many values at a
rounding boundary, and the float64 descriptor orders a rotated ellipse before every other shape.  No GPU."""
import numpy as np
import pytest
import torch

import lfd_cases as lc

NON_EMPTY = [k for k in lc.CASES if not k.startswith("empty")]


def test_rotation_perms_are_the_rotation_group_acting_on_the_vertex_pairs():
    from meshdiffusion_amd import lfd
    perms = lfd.rotation_perms()
    assert perms.dtype == np.uint8 and perms.shape == (60, 10)
    rows = [tuple(int(v) for v in r) for r in perms]
    assert all(sorted(r) == list(range(10)) for r in rows)
    assert len(set(rows)) == 60 and rows[0] == tuple(range(10))
    have = set(rows)
    for a in rows:
        inverse = [0] * 10
        for v, u in enumerate(a):
            inverse[u] = v
        assert tuple(inverse) in have
        for b in rows:
            assert tuple(a[b[v]] for v in range(10)) in have
    # the table is the action of `rotation_matrices` on `view_directions`
    d, mats = lfd.view_directions(), lfd.rotation_matrices()
    assert d.shape == (10, 3) and d.dtype == np.float64 and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-15)
    for g in (0, 7, 59):
        assert np.allclose(np.abs(np.sum((d @ mats[g].T) * d[perms[g]], axis=1)), 1.0, atol=1e-12)
    assert np.allclose(mats @ mats.transpose(0, 2, 1), np.eye(3), atol=1e-12) and np.allclose(np.linalg.det(mats), 1.0)


def test_view_directions_are_the_documented_vertex_pairs():
    from meshdiffusion_amd import lfd
    phi = (1 + 5 ** 0.5) / 2
    d = lfd.view_directions() * 3 ** 0.5
    assert np.allclose(d[0], (1, 1, 1)) and np.allclose(d[3], (1, -1, -1)) and np.allclose(d[4], (0, 1 / phi, phi))
    assert np.allclose(d[7], (phi, 0, -1 / phi)) and np.allclose(d[9], (1 / phi, -phi, 0))
    gram = np.abs(d @ d.T) / 3                       # no two directions are parallel: ten different pairs
    assert (gram - np.eye(10)).max() < 0.75
    frames = lfd.view_frames()
    assert np.allclose(frames @ frames.transpose(0, 2, 1), np.eye(3), atol=1e-12) and np.allclose(frames[:, 2], lfd.view_directions())


def test_light_fields_are_more_than_five_degrees_apart_modulo_the_group():
    from meshdiffusion_amd import lfd
    F, G = lfd.field_rotations(10), lfd.rotation_matrices()
    assert np.array_equal(F[0], np.eye(3)) and np.allclose(F @ F.transpose(0, 2, 1), np.eye(3), atol=1e-12)
    worst = 180.0
    for j in range(10):
        for k in range(j):
            tr = np.trace(np.einsum("ab,cb,gcd->gad", F[j], F[k], G), axis1=1, axis2=2)      # R_j R_k^T g
            worst = min(worst, float(np.degrees(np.arccos(np.clip((tr - 1) / 2, -1, 1))).min()))
    print(f"\nsmallest angle between two light fields modulo the 60 rotations: {worst:.2f} degrees")
    assert worst > 5.0
    with pytest.raises(ValueError):
        lfd.field_rotations(17)


def test_fp32_scheme_stays_inside_the_bar_of_float64():
    worst, where = 0.0, None
    for name in NON_EMPTY:
        c64 = lc.reference(name)[0]
        share = np.abs(lc.describe_fp32(lc.CASES[name]).astype(np.float64) - c64) / lc.COEF_BAR
        if share.max() > worst:
            worst, where = float(share.max()), (name, int(share.argmax()))
        assert bool((share <= 1).all()), (name, int(share.argmax()), float(share.max()))
    print(f"\nfp32 restatement: worst share of the bar {worst:.3f} at {where}")


def test_bar_follows_the_coefficient_sums():
    assert lc.radial_coefficients(10, 0) == [(252, 10), (-630, 8), (560, 6), (-210, 4), (30, 2), (-1, 0)]
    assert lc.radial_coefficients(4, 2) == [(4, 4), (-3, 2)] and lc.radial_coefficients(7, 7) == [(1, 7)]
    for n, m in lc.NM:                               # R_nm(1) = 1
        assert sum(c for c, _ in lc.radial_coefficients(n, m)) == 1
    assert lc.DESC_BAR[10, 0] == 512 * (1.001 * 2.0 ** -24 * 1683 * 26 + 2.0 ** -32) + 512 * 2.0 ** -24
    assert max(lc.DESC_BAR.values()) == lc.DESC_BAR[10, 0] and min(lc.DESC_BAR.values()) == lc.DESC_BAR[1, 1]


def test_cases_keep_clear_of_bin_and_rounding_boundaries():
    clear = {name: lc.bin_clearance(lc.CASES[name]) for name in NON_EMPTY}
    tight = min(clear, key=clear.get)
    near = np.stack([lc.near_half(lc.reference(name)[0]) for name in NON_EMPTY])
    print(f"\nsmallest bin clearance {clear[tight]:.3e} bins ({tight}); {near.mean() * 100:.1f} % of the values within the bar of a half-integer")
    assert clear[tight] > 2.0 ** -16
    assert near.mean() <= 0.15


def test_empty_and_floor_cases_in_float64():
    coef, desc, status = lc.reference("empty16")
    assert status == 1 and not desc.any() and not coef.any()
    coef, desc, status = lc.reference("pixel16")     # rho = 0: R_n0(0) = +-1, everything else 0; no signature
    assert status == 0
    for k, (n, m) in enumerate(lc.NM):
        assert coef[k] == (512.0 if m == 0 else 0.0)
    assert not coef[35:].any() and not desc[45:].any()
    coef, _, _ = lc.reference("pair16")              # both pixels at rho = 1 (rmax at its floor 0.5): R_nm(1) = 1, m even survive
    for k, (n, m) in enumerate(lc.NM):
        assert abs(coef[k] - (512.0 if m % 2 == 0 else 0.0)) < 1e-9


def test_float64_descriptor_orders_a_rotated_ellipse_first():
    def sad(a, b):
        return int(np.abs(lc.reference(a)[1].astype(np.int64) - lc.reference(b)[1].astype(np.int64)).sum())
    rotated = sad("ellipse256", "ellipse256_rot")
    others = {k: sad("ellipse256", k) for k in lc.CASES if k.endswith("256") and not k.startswith("ellipse")}
    print(f"\nellipse against itself turned by 0.6 rad: {rotated}; nearest other shape: {min(others.values())} ({min(others, key=others.get)})")
    assert rotated < min(others.values())


def test_matrix_restatement_on_hand_made_models():
    x = np.zeros((1, 1, 10, 48), dtype=np.uint8)
    y = np.full((1, 1, 10, 48), 255, dtype=np.uint8)
    ident = np.arange(10)[None]
    assert lc.matrix_numpy(x, y, ident)[0, 0] == 10 * 48 * 255 == 122400
    x = lc.random_models(1, 1, 5)
    shift = np.roll(np.arange(10), 1)[None]
    y = np.zeros_like(x)
    y[0, 0, shift[0]] = x[0, 0]                       # y[perm[v]] = x[v]
    assert lc.matrix_numpy(x, y, shift)[0, 0] == 0 and lc.matrix_numpy(x, y, ident)[0, 0] > 0


def test_lfd_host_checks():
    from meshdiffusion_amd import _lib, lfd
    desc = torch.zeros((2, 10, 10, 48), dtype=torch.uint8)
    for call in (lambda: lfd.lfd_matrix(desc), lambda: lfd.lfd_metrics(desc, desc), lambda: lfd.describe(torch.zeros((1, 8, 8), dtype=torch.uint8)),
                 lambda: lfd.silhouettes(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int64))):
        with pytest.raises(_lib.MeshDiffusionHipError, match="GPU only"):
            call()
    for bad in (torch.zeros((2, 10, 9, 48), dtype=torch.uint8), torch.zeros((2, 10, 10, 47), dtype=torch.uint8),
                torch.zeros((0, 10, 10, 48), dtype=torch.uint8), torch.zeros((2, 17, 10, 48), dtype=torch.uint8),
                torch.zeros((2, 10, 10, 48), dtype=torch.int32), torch.zeros((2, 10, 480), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            lfd.lfd_matrix(bad)
    # perms are checked before anything touches a device
    for perms in (np.full((1, 10), 10), np.zeros((65, 10), dtype=np.uint8), np.zeros((0, 10), dtype=np.uint8), np.zeros((3, 9), dtype=np.uint8),
                  np.zeros((2, 10), dtype=np.float32), -np.ones((1, 10), dtype=np.int64)):
        with pytest.raises(ValueError, match="perms"):
            lfd._perms(perms)
    assert lfd._perms(None).shape == (60, 10) and lfd._perms(None).dtype == torch.uint8
    with pytest.raises(ValueError):
        lfd.describe(torch.zeros((1, 8, 9), dtype=torch.uint8))
    with pytest.raises(ValueError):
        lfd.lfd_descriptors([(np.zeros((3, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int64))])
    assert (lfd.VIEWS, lfd.DESC_BYTES, lfd.COEFS, lfd.MAX_RES, lfd.MAX_FIELDS, lfd.MAX_ROTATIONS) == (10, 48, 45, 512, 16, 64)


def test_export_refuses_bad_arguments_on_the_host(hip_lib):
    """md_lfd_matrix reads `perm` on the host and returns before any launch; so do the limits of md_lfd_describe."""
    import ctypes as C
    from meshdiffusion_amd import _lib
    buf = (C.c_uint8 * 4800)()
    out = (C.c_int32 * 4)()
    p = C.cast(buf, C.c_void_p)
    o = C.cast(out, C.c_void_p)
    good = (C.c_uint8 * 10)(*range(10))
    bad = (C.c_uint8 * 10)(0, 1, 2, 3, 4, 5, 6, 7, 8, 10)
    assert hip_lib.md_lfd_matrix(p, p, C.cast(bad, C.c_void_p), 1, 1, 1, 1, 0, o, None) == _lib.ERR_BAD_ARG
    assert hip_lib.md_lfd_matrix(p, p, C.cast(good, C.c_void_p), 1, 1, 17, 1, 0, o, None) == _lib.ERR_UNSUPPORTED
    assert hip_lib.md_lfd_matrix(p, p, C.cast(good, C.c_void_p), 1, 1, 1, 65, 0, o, None) == _lib.ERR_UNSUPPORTED
    assert hip_lib.md_lfd_matrix(p, p, C.cast(good, C.c_void_p), 1, 0, 1, 1, 0, o, None) == _lib.ERR_BAD_ARG
    assert hip_lib.md_lfd_matrix(p, p, C.cast(good, C.c_void_p), 1, 2, 1, 1, 1, o, None) == _lib.ERR_BAD_ARG
    assert hip_lib.md_lfd_matrix(p, None, C.cast(good, C.c_void_p), 1, 1, 1, 1, 0, o, None) == _lib.ERR_BAD_ARG
    assert hip_lib.md_lfd_describe(p, 1, 513, p, None, o, None) == _lib.ERR_UNSUPPORTED
    assert hip_lib.md_lfd_describe(p, 0, 16, p, None, o, None) == _lib.ERR_BAD_ARG
    assert hip_lib.md_lfd_describe(None, 1, 16, p, None, o, None) == _lib.ERR_BAD_ARG
