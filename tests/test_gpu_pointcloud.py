"""Point-cloud kernels on the GPU: md_nn_sided, md_chamfer_bwd, md_face_areas, md_sample_points(+_bwd) and the fitting loop
built on them, against the float64 restatements of tests/pointcloud_cases.py and the reference data of
tests/golden/pointcloud.npz.  The float64 oracles run on the GPU too (torch float64 brute force).

Bars, none fitted to what the kernels give:
  nearest neighbours   |d2_gpu - d2_64| <= 2^-20 d2_64 for EVERY query (pointcloud_cases.NN_VALUE_BAR: direct-form evaluation
                       5 * 2^-24, a neighbour that is nearest in fp32 only 10 * 2^-24, rounded up to 16 * 2^-24); the index
                       equals the float64 index outside the near-tie set that tests/test_cpu_pointcloud_host.py proves rare,
                       and everywhere on the exact-tie cases.
  chamfer, d verts     the fp32 torch restatement's OWN rel-L2 distance from float64 on the same case, recorded in the fixture
                       by the generator, x 4 (as tests/test_gpu_dmtet_grad.py).
  sampled points       4 * 2^-24 * max|coordinate| from the unmodified reference's points (three products and two sums).
  per-face counts      5 sigma of the binomial expectation from the float64 areas.
  fitting run          4 x |fp32 - float64| of the reference loop at each stored iteration.
Each test prints its figures before it asserts.
"""
import os

import numpy as np
import pytest
import torch

import pointcloud_cases as pc
from conftest import GOLD

pytestmark = pytest.mark.gpu
BAR = 4.0
CLAMP = float(torch.tensor(0.99))         # clamp_deform's bound as the float32 it is stored in (above the double 0.99)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "pointcloud.npz"))


@pytest.fixture(scope="module")
def tet():
    t = np.load(os.path.join(GOLD, "64_tets_cropped.npz"))
    return t["vertices"], t["indices"]


def _check_nn(name, dist, idx, d1, i1, d2, exact):
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.shape == d1.shape and idx.shape == d1.shape
    err = (dist.double() - d1).abs()
    worst = float((err / d1.clamp_min(1e-300)).max()) if bool((d1 > 0).any()) else 0.0
    near = pc.near_tie(d1, d2)
    wrong = idx != i1
    print(f"\n{name}: queries {d1.numel()} worst |d2 - d2_64| / d2_64 {worst:.3e} (bar {pc.NN_VALUE_BAR:.3e}) near ties "
          f"{int(near.sum())} index differences {int(wrong.sum())} (outside the near-tie set {int((wrong & ~near).sum())})")
    assert bool((err <= pc.NN_VALUE_BAR * d1).all()), name
    if exact:
        assert not bool(wrong.any()), name
    else:
        assert not bool((wrong & ~near).any()), name
    assert int(idx.min()) >= 0


@pytest.mark.parametrize("name", pc.NN_CASES)
def test_nn_sided_against_float64(hip_lib, name):
    from meshdiffusion_amd.pointcloud import sided_distance
    p, q, skip = pc.nn_case(name)
    p = p.cuda()
    q = p if q is None else q.cuda()
    dist, idx = sided_distance(p, q, skip_same_index=skip)
    d1, i1, d2 = pc.nn_float64(p, None if skip else q, skip)
    _check_nn(name, dist, idx, d1, i1, d2, name in pc.EXACT_TIE_CASES)
    again = sided_distance(p, q, skip_same_index=skip)
    assert torch.equal(dist, again[0]) and torch.equal(idx, again[1])            # bit-identical from run to run
    if skip:
        ar = torch.arange(p.shape[1], device="cuda")
        assert not bool((idx == ar[None]).any())                                 # never itself
    if name == "dups":
        assert bool((dist[0, :500] == 0).all()) and bool((dist[0, 2000:] == 0).all())
    if name == "spheres":                                                        # the other direction at the real size
        dist, idx = sided_distance(q, p)
        _check_nn("spheres (reverse)", dist, idx, *pc.nn_float64(q, p), False)


def test_nn_sided_without_skip_finds_itself(hip_lib):
    from meshdiffusion_amd.pointcloud import sided_distance
    p = pc.nn_case("self")[0].cuda()
    dist, idx = sided_distance(p, p)
    assert not bool(dist.any()) and torch.equal(idx[0], torch.arange(p.shape[1], device="cuda"))


def test_nn_sided_non_finite_coordinates(hip_lib):
    """A NaN in one query point gives a NaN distance for that query only; a NaN candidate wins for every query (torch.min);
    an infinite query is infinitely far from every finite candidate."""
    from meshdiffusion_amd.pointcloud import sided_distance
    p, q, _ = pc.nn_case("unequal")
    p, q = p.cuda().clone(), q.cuda()
    clean = sided_distance(p, q)
    p[0, 77, 1] = float("nan")
    p[0, 1100, 0] = float("inf")
    dist, idx = sided_distance(p, q)
    bad = torch.zeros(p.shape[1], dtype=torch.bool, device="cuda")
    bad[77] = bad[1100] = True
    assert bool(torch.isnan(dist[0, 77])) and float(dist[0, 1100]) == float("inf") and int(idx[0, 1100]) == 0
    assert int(idx[0, 77]) == 0                                                  # torch.min's index of the first NaN
    assert torch.equal(dist[0, ~bad], clean[0][0, ~bad]) and torch.equal(idx[0, ~bad], clean[1][0, ~bad])
    assert int(torch.isnan(dist).sum()) == 1
    q2 = q.clone()
    q2[0, 2500, 2] = float("nan")
    dist, idx = sided_distance(pc.nn_case("unequal")[0].cuda(), q2)
    assert bool(torch.isnan(dist).all()) and bool((idx == 2500).all())
    want = torch.min(((pc.nn_case("unequal")[0].cuda()[0, :, None] - q2[0, None]) ** 2).sum(-1), dim=1)
    assert bool(torch.isnan(want.values).all())


@pytest.mark.parametrize("name", pc.CHAMFER_CASES)
def test_chamfer_distance_value_and_gradients(hip_lib, gold, name):
    from meshdiffusion_amd.pointcloud import chamfer_distance
    p, q, w1, w2 = pc.chamfer_case(name)
    p, q = p.cuda(), q.cuda()
    g = pc.chamfer_cotangent(p.shape[0]).cuda()

    def run(q_grad=True):
        a, b = p.clone().requires_grad_(True), q.clone().requires_grad_(q_grad)
        val = chamfer_distance(a, b, w1, w2)
        assert val.shape == (p.shape[0],) and val.dtype == torch.float32
        (val * g).sum().backward()
        return val.detach(), a.grad, b.grad

    val, dp, dq = run()
    _, i12, _ = pc.nn_float64(p, q)
    _, i21, _ = pc.nn_float64(q, p)
    v64, a64, b64 = pc.chamfer_restated(p, q, w1, w2, i12, i21, torch.float64, g)
    assert float((v64.cpu() - torch.as_tensor(gold[f"chamfer/{name}/value64"])).abs().max()) <= 1e-12
    ev, ea, eb = pc.rel_l2(val, v64), pc.rel_l2(dp, a64), pc.rel_l2(dq, b64)
    bv, ba, bb = (BAR * float(gold[f"chamfer/{name}/ref_err_{k}"]) for k in ("value", "dp1", "dp2"))
    print(f"\nchamfer {name}: value {val.tolist()} vs float64 {ev:.3e} (bar {bv:.3e}) dp1 {ea:.3e} (bar {ba:.3e}) dp2 {eb:.3e} (bar {bb:.3e})")
    assert ev <= bv and ea <= ba and eb <= bb
    v2, dp2, dq2 = run()
    assert torch.equal(val, v2) and torch.equal(dp, dp2) and torch.equal(dq, dq2)          # bit-equal across two calls
    v3, dp3, dq3 = run(q_grad=False)
    assert dq3 is None and torch.equal(dp3, dp) and torch.equal(v3, val)
    with pytest.raises(NotImplementedError):
        chamfer_distance(p, q, squared=False)


def _sample_inputs(gold, name):
    verts, faces = pc.sample_case(name)
    ch = torch.as_tensor(gold[f"sample/{name}/choices"].astype(np.int64))
    r_u, r_v = torch.as_tensor(gold[f"sample/{name}/r_u"]), torch.as_tensor(gold[f"sample/{name}/r_v"])
    return verts.cuda(), faces.cuda(), ch.cuda(), r_u.cuda(), r_v.cuda()


@pytest.mark.parametrize("name", pc.SAMPLE_CASES)
def test_sample_points_given_faces_match_the_reference_points(hip_lib, gold, name):
    from meshdiffusion_amd.pointcloud import sample_points
    verts, faces, ch, r_u, r_v = _sample_inputs(gold, name)
    B, S = ch.shape
    pts, got_ch = sample_points(verts, faces, S, uniforms=(None, r_u, r_v), face_choices=ch)
    assert pts.shape == (B, S, 3) and pts.dtype == torch.float32 and got_ch.shape == (B, S) and got_ch.dtype == torch.int64
    assert torch.equal(got_ch, ch)
    want = torch.as_tensor(gold[f"sample/{name}/points"]).cuda()
    err, bound = float((pts.double() - want.double()).abs().max()), 4 * 2.0 ** -24 * float(verts.abs().max())
    print(f"\nsample {name}: max|points - reference| {err:.3e} (bound {bound:.3e}) bit-equal rows {int((pts == want).all(-1).sum())} / {B * S}")
    assert err <= bound
    # face features: interpolated with the same weights
    D = 2
    ff = pc.case_G((B, faces.shape[0], 3, D), 77).cuda()
    pts2, ch2, feats = sample_points(verts, faces, S, face_features=ff, uniforms=(None, r_u, r_v), face_choices=ch)
    assert torch.equal(pts2, pts) and torch.equal(ch2, ch) and feats.shape == (B, S, D)
    _, w = pc.sample_points_restated(verts, faces, ch, r_u, r_v)
    sel = ff.double()[torch.arange(B, device="cuda")[:, None], ch]
    want_f = (w[..., None] * sel).sum(2)
    assert float((feats.double() - want_f).abs().max()) <= 4 * 2.0 ** -24 * float(ff.abs().max())


@pytest.mark.parametrize("name", pc.SAMPLE_CASES)
def test_sample_points_inverse_cdf(hip_lib, name):
    from meshdiffusion_amd.pointcloud import face_areas, sample_points
    verts, faces = pc.sample_case(name)
    verts, faces = verts.cuda(), faces.cuda()
    B, S = verts.shape[0], pc.SAMPLE_SIZES[name] * 8
    uni = tuple(t.cuda() for t in pc.case_uniforms(B, S, pc.SAMPLE_SEEDS[name] + 7))
    areas64 = pc.face_areas_restated(verts, faces)
    areas = face_areas(verts, faces)
    ea = float(((areas.double() - areas64).abs() / areas64.max()).max())
    assert areas.shape == areas64.shape and ea <= 8 * 2.0 ** -24 and torch.equal(areas == 0, areas64 == 0)
    pts, ch = sample_points(verts, faces, S, uniforms=uni)
    want, near = pc.face_choices_restated(areas64, uni[0])
    diff = ch != want
    print(f"\ninverse CDF {name}: areas vs float64 {ea:.2e} samples {B * S} near a boundary {int(near.sum())} different faces "
          f"{int(diff.sum())} (outside the near set {int((diff & ~near).sum())})")
    assert not bool((diff & ~near).any())
    assert bool((areas64.gather(1, ch) > 0).all())                               # never a zero-area face
    p64, _ = pc.sample_points_restated(verts, faces, ch, uni[1], uni[2])
    assert float((pts.double() - p64).abs().max()) <= 4 * 2.0 ** -24 * float(verts.abs().max())
    again = sample_points(verts, faces, S, uniforms=uni)
    assert torch.equal(again[0], pts) and torch.equal(again[1], ch)
    given = sample_points(verts, faces, S, areas=areas, uniforms=torch.stack(uni))
    assert torch.equal(given[0], pts) and torch.equal(given[1], ch)


def test_sample_points_face_counts_follow_the_areas(hip_lib):
    """10^6 samples on a mesh whose areas span five orders of magnitude: every face's count within 5 sigma of its binomial
    expectation (sigma from the float64 areas), the zero-area face never."""
    from meshdiffusion_amd.pointcloud import sample_points
    verts, faces = pc.unequal_mesh()
    verts, faces = verts.cuda(), faces.cuda()
    S = 1_000_000
    uni = tuple(t.cuda() for t in pc.case_uniforms(1, S, 5399))
    _, ch = sample_points(verts, faces, S, uniforms=uni)
    a = pc.face_areas_restated(verts, faces)[0]
    prob = a / a.sum()
    count = torch.bincount(ch[0], minlength=faces.shape[0]).double()
    sigma = torch.sqrt(S * prob * (1 - prob))
    z = (count - S * prob).abs() / sigma.clamp_min(1e-300)
    print(f"\ncounts {count.tolist()}\nexpected {(S * prob).tolist()}\n|z| {z.tolist()}")
    assert bool((count[a == 0] == 0).all()) and bool((count[a > 0] > 0).all())
    assert bool((z[a > 0] <= 5).all())
    # the default path draws its own uniforms on the device; a generator makes it repeatable
    g1, g2 = torch.Generator(device="cuda").manual_seed(5), torch.Generator(device="cuda").manual_seed(5)
    x, y = sample_points(verts, faces, 4096, generator=g1), sample_points(verts, faces, 4096, generator=g2)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[0].shape == (1, 4096, 3)


@pytest.mark.parametrize("name", pc.SAMPLE_CASES)
def test_sample_points_backward(hip_lib, gold, name):
    from meshdiffusion_amd.pointcloud import sample_points
    verts, faces, ch, r_u, r_v = _sample_inputs(gold, name)
    B, S = ch.shape
    G = pc.case_G((B, S, 3), pc.SAMPLE_SEEDS[name] + 50).cuda()

    def run():
        v = verts.clone().requires_grad_(True)
        pts, _ = sample_points(v, faces, S, uniforms=(None, r_u, r_v), face_choices=ch)
        assert pts.requires_grad
        (pts * G).sum().backward()
        return v.grad

    dv = run()
    want = pc.sample_points_grad_restated(verts, faces, ch, r_u, r_v, G)
    e, bar = pc.rel_l2(dv, want), BAR * float(gold[f"sample/{name}/ref_err_grad"])
    print(f"\nsample backward {name}: d verts vs float64 {e:.3e} (bar {bar:.3e})")
    assert dv.shape == verts.shape and dv.dtype == torch.float32 and e <= bar
    assert torch.equal(dv, run())                                                # bit-equal across two calls
    untouched = torch.ones(B, verts.shape[1], dtype=torch.bool, device="cuda")
    untouched[torch.arange(B, device="cuda")[:, None, None], faces[ch]] = False
    assert not bool(dv[untouched].any())                                         # exactly zero where no sample landed
    # through the inverse CDF as well: the face choice is not differentiated
    uni = tuple(t.cuda() for t in pc.case_uniforms(B, S, 31))
    v = verts.clone().requires_grad_(True)
    pts, ch2 = sample_points(v, faces, S, uniforms=uni)
    (pts * G).sum().backward()
    want = pc.sample_points_grad_restated(verts, faces, ch2, uni[1], uni[2], G)
    assert pc.rel_l2(v.grad, want) <= bar


def test_vert_nn_dist_of_the_shipped_grid(hip_lib, tet):
    from meshdiffusion_amd.dmtet import DMTetGeometry
    verts, idx = tet
    geo = DMTetGeometry(64, 2.1, None, tets=(verts, idx), deform_scale=2.0)
    with torch.no_grad():
        geo.deform.copy_(pc.case_G(tuple(geo.deform.shape), 41).cuda() * 0.5)
    d = geo.getVertNNDist()
    assert d.shape == (verts.shape[0],) and d.dtype == torch.float32 and not d.requires_grad
    v = (geo.verts + 2 / (64 * 2) * torch.tanh(geo.deform)).detach()[None]
    d1, i1, d2 = pc.nn_float64(v, None, True)
    err = (d.double() - d1[0]).abs()
    print(f"\ngetVertNNDist: N={d.numel()} worst relative error {float((err / d1[0]).max()):.3e} (bar {pc.NN_VALUE_BAR:.3e})")
    assert bool((err <= pc.NN_VALUE_BAR * d1[0]).all()) and float(d.min()) > 0
    # the small torch members of the class
    c = geo.getTetCenters()
    assert c.shape == (idx.shape[0], 3) and torch.allclose(c, geo.get_deformed()[geo.indices].mean(1))
    with torch.no_grad():
        geo.sdf.copy_(0.5 - geo.verts.norm(dim=1))
    mesh = geo.getMesh()
    vt = geo.getValidTetIdx()
    assert vt.dtype == torch.int64 and vt.shape[0] == mesh.t_pos_idx.shape[0]
    assert torch.equal(geo.getValidVertsIdx(), mesh.valid_vert_idx)
    with torch.no_grad():
        geo.deform.mul_(10)
        geo.sdf.mul_(10)
    geo.clamp_deform()
    assert float(geo.deform.abs().max()) <= CLAMP and float(geo.sdf.abs().max()) <= 1.0


def test_fit_to_points_end_to_end(hip_lib, tet, gold):
    """fit_to_points on the shipped 64 tet grid to FIT_TARGET_POINTS points of a sphere of radius 0.6 from a sphere of radius 0.45
    (pointcloud_cases.fit_initial_sdf says why not the reference's random start), explicit per-iteration uniforms, 41 iterations; then state_to_dict -> tet_to_grid.
    Bar: within 4 x |fp32 - float64| of the float64 value of the reference loop at iterations 0, 10, 20, 40."""
    from meshdiffusion_amd import mesh_export
    from meshdiffusion_amd.dmtet import DMTetGeometry, tet_vertices_to_grid_index
    from meshdiffusion_amd.pointcloud import fit_to_points
    verts, idx = tet
    geo = DMTetGeometry(64, 2.1, None, tets=(verts, idx), deform_scale=2.0)
    with torch.no_grad():
        geo.sdf.copy_(pc.fit_initial_sdf(geo.verts))
        geo.deform.zero_()
    seen = []
    hist = fit_to_points(geo, pc.fit_target().cuda(), pc.FIT_ITERS, num_samples=pc.FIT_SAMPLES, lr=pc.FIT_LR,
                         sdf_regularizer=pc.FIT_SDF_REGULARIZER, uniforms=lambda it: tuple(t.cuda() for t in pc.fit_uniforms(it)),
                         callback=lambda it, c, mesh: seen.append(it))
    assert hist.shape == (pc.FIT_ITERS,) and hist.dtype == torch.float32 and seen == list(range(pc.FIT_ITERS))
    got = hist.double().cpu().numpy()[list(pc.FIT_STEPS)]
    l32, l64 = gold["fit/loss32"], gold["fit/loss64"]
    unit = np.abs(l32 - l64)
    ratio = np.abs(got - l64) / unit
    print(f"\nfit: chamfer {got} float64 reference {l64} fp32 reference {l32} |gpu - f64| / |f32 - f64| {ratio}")
    assert got[3] < 0.5 * got[0]
    assert (ratio <= BAR).all()
    d = geo.state_to_dict()
    assert set(d) == {"sdf", "deform"} and float(d["deform"].abs().max()) <= CLAMP and float(d["sdf"].abs().max()) <= 1.0
    gi = tet_vertices_to_grid_index(torch.as_tensor(verts))
    grid = mesh_export.tet_to_grid(gi, d["sdf"], d["deform"], 64)
    assert tuple(grid.shape) == (4, 64, 64, 64)
    mask = torch.zeros(64, 64, 64, dtype=torch.bool)
    mask[gi[:, 0], gi[:, 1], gi[:, 2]] = True
    assert not bool(torch.as_tensor(grid)[:, ~mask].any()) and bool(torch.as_tensor(grid)[:, mask].any())
