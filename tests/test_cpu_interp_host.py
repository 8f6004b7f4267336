"""Host side of the attribute interpolation, the barycentric backward, the vertex normals and the `bsdf == 'normal'` renderer
(meshdiffusion_amd/render.py, meshdiffusion_amd/dmtet.py, csrc/interp.hip) without a GPU: the export tables, argument refusal, the
plain-torch parts against float64 formulas, and the restatements of tests/interp_cases.py against themselves -- central
differences against their autograd, a face-constant attribute, the mask."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import antialias_cases as ac
import interp_cases as ic
import raster_cases as rc
from conftest import GOLD, ROOT

SMALL = ic.CASES[3:]                   # quad, fan40, degen at 16 x 16


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "interp.npz"))


def test_new_exports_are_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import build, dmtet, render
    assert "interp.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "interp.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "THE INTERPOLATION CONTRACT" in src and "atomicAdd" not in src
    for name in ("interpolate", "shading_normal", "render_buffers", "image_loss", "color_loss"):
        assert callable(getattr(render, name)), name
    assert callable(dmtet.vertex_normals)


def test_new_exports_refuse_bad_arguments_without_a_gpu(hip_lib):
    nul, one, odd8, odd4 = C.c_void_p(0), C.c_void_p(64), C.c_void_p(72), C.c_void_p(68)

    def refuses(fn, ok, pointers, sizes):
        for k in pointers:
            a = list(ok); a[k] = nul
            assert fn(*a) == -1, (fn.__name__, k)
        for k in sizes:
            for bad in (0, -3):
                a = list(ok); a[k] = bad
                assert fn(*a) == -1, (fn.__name__, k, bad)

    def unsupported(fn, ok, cases):
        for k, v in cases:
            a = list(ok); a[k] = v
            assert fn(*a) == -2, (fn.__name__, k, v)

    def misaligned(fn, ok, cases):
        for k, p in cases:
            a = list(ok); a[k] = p
            assert fn(*a) == -1, (fn.__name__, k)

    # md_interpolate(rast, attr, tri, B, Ba, N, C, F, H, W, out, stream)
    ok = [one, one, one, 2, 1, 100, 3, 300, 64, 48, one, nul]
    refuses(hip_lib.md_interpolate, ok, (0, 1, 2, 10), (3, 4, 5, 7, 8, 9))
    unsupported(hip_lib.md_interpolate, ok, ((6, 0), (6, 9), (6, -1), (3, 65), (7, 1 << 24), (8, 2049), (9, 2049)))
    misaligned(hip_lib.md_interpolate, ok, ((0, odd8), (2, odd4)))
    a = list(ok); a[4] = 3
    assert hip_lib.md_interpolate(*a) == -1                           # Ba is 1 or B
    # md_interpolate_bwd(cov, n_cov, rast, grad_out, attr, tri, ptr, order, B, Ba, N, C, F, H, W, corner_grad, dattr, drast, stream)
    ok = [one, 500, one, one, one, one, one, one, 2, 1, 100, 3, 300, 64, 48, one, one, one, nul]
    refuses(hip_lib.md_interpolate_bwd, ok, (0, 2, 3, 4, 5, 6, 7, 15), (8, 9, 10, 12, 13, 14))
    unsupported(hip_lib.md_interpolate_bwd, ok, ((11, 0), (11, 9), (8, 65), (12, 1 << 24), (13, 2049), (14, 2049)))
    misaligned(hip_lib.md_interpolate_bwd, ok, ((2, odd8), (17, odd8), (5, odd4)))
    a = list(ok); a[1] = -1
    assert hip_lib.md_interpolate_bwd(*a) == -1
    a = list(ok); a[16] = a[17] = nul
    assert hip_lib.md_interpolate_bwd(*a) == -1                       # nothing to compute
    a = list(ok); a[1] = (1 << 30)
    assert hip_lib.md_interpolate_bwd(*a) == -2                       # 3 n_cov must fit the int32 codes
    a = list(ok); a[8], a[9], a[10] = 64, 64, 1 << 26
    assert hip_lib.md_interpolate_bwd(*a) == -2                       # Ba N must fit the int32 CSR
    # md_raster_bary_bwd(cov, n_cov, rast, drast, pos_clip, faces, ptr, order, B, V, F, H, W, corner_grad, dpos_clip, stream)
    ok = [one, 500, one, one, one, one, one, one, 2, 100, 300, 64, 48, one, one, nul]
    refuses(hip_lib.md_raster_bary_bwd, ok, (0, 2, 3, 4, 5, 6, 7, 13, 14), (8, 9, 10, 11, 12))
    unsupported(hip_lib.md_raster_bary_bwd, ok, ((8, 65), (10, 1 << 24), (11, 2049), (12, 2049)))
    misaligned(hip_lib.md_raster_bary_bwd, ok, ((2, odd8), (3, odd8), (4, odd8), (14, odd8), (5, odd4)))
    a = list(ok); a[1] = -1
    assert hip_lib.md_raster_bary_bwd(*a) == -1
    a = list(ok); a[1] = (1 << 30)
    assert hip_lib.md_raster_bary_bwd(*a) == -2
    a = list(ok); a[8], a[9] = 64, 1 << 26
    assert hip_lib.md_raster_bary_bwd(*a) == -2                       # B V must fit the int32 CSR
    # md_vertex_normals_det(verts, faces, ptr, order, V, F, v_nrm, f_nrm, v_len, stream)
    ok = [one, one, one, one, 100, 300, one, one, one, nul]
    refuses(hip_lib.md_vertex_normals_det, ok, (0, 1, 2, 3, 6, 7, 8), (4, 5))
    unsupported(hip_lib.md_vertex_normals_det, ok, ((5, 1 << 24),))
    misaligned(hip_lib.md_vertex_normals_det, ok, ((1, odd4),))
    # md_vertex_normals_bwd(verts, faces, ptr, order, v_nrm, v_len, grad_v_nrm, V, F, face_grad, dverts, stream)
    ok = [one, one, one, one, one, one, one, 100, 300, one, one, nul]
    refuses(hip_lib.md_vertex_normals_bwd, ok, (0, 1, 2, 3, 4, 5, 6, 9, 10), (7, 8))
    unsupported(hip_lib.md_vertex_normals_bwd, ok, ((8, 1 << 24),))
    misaligned(hip_lib.md_vertex_normals_bwd, ok, ((1, odd4),))


def test_host_functions_check_their_arguments():
    from meshdiffusion_amd import _lib, dmtet, render
    rast, attr, tri = torch.zeros(1, 8, 8, 4), torch.zeros(4, 3), torch.tensor([[0, 1, 2]])
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.interpolate(attr, rast, tri)                             # CPU tensors: no fallback
    with pytest.raises(_lib.MeshDiffusionHipError):
        dmtet.vertex_normals(attr, tri)
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.render_buffers(attr, tri, torch.eye(4)[None], torch.zeros(1, 3), 8)
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.rasterize(torch.zeros(1, 4, 4), tri, 8, grad=True)
    with pytest.raises(ValueError):
        render.image_loss(rast, rast, "l7")
    geo = type("G", (), {"sdf": torch.zeros(3)})()
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.fit_to_views(geo, {}, 1, color_weight=1.0)


def test_shape_checks_come_before_any_launch(monkeypatch):
    """With the GPU test of the entry points switched off, bad shapes, channel counts and indices are refused on the host."""
    from meshdiffusion_amd import _lib, render
    monkeypatch.setattr(render, "_gpu_only", lambda t, what: None)
    rast, tri = torch.zeros(2, 8, 8, 4), torch.tensor([[0, 1, 2]])
    for bad_attr in (torch.zeros(3, 4, 3), torch.zeros(4), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError):
            render.interpolate(bad_attr, rast, tri)
    with pytest.raises(ValueError):
        render.interpolate(torch.zeros(4, 3), torch.zeros(2, 8, 8, 3), tri)
    with pytest.raises(ValueError):
        render.interpolate(torch.zeros(4, 3), rast, torch.tensor([[0, 1, 4]]))   # index outside the attribute rows
    with pytest.raises(ValueError):
        render.interpolate(torch.zeros(4, 3), rast, torch.tensor([[0, 1]]))
    for C_bad in (0, 9):
        with pytest.raises(_lib.MeshDiffusionHipError):
            render.interpolate(torch.zeros(4, C_bad), rast, tri)
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.interpolate(torch.zeros(4, 3), torch.zeros(65, 2, 2, 4), tri)
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.interpolate(torch.zeros(4, 3), torch.zeros(1, 2049, 1, 4), tri)


@pytest.mark.parametrize("kind", ic.LOSS_KINDS)
def test_image_loss_matches_the_restated_formula(kind):
    from meshdiffusion_amd import render
    gen = torch.Generator().manual_seed(11)
    img, ref = torch.rand(2, 9, 7, 3, generator=gen) * 1.5 - 0.1, torch.rand(2, 9, 7, 3, generator=gen)
    got, want = float(render.image_loss(img, ref, kind)), float(ic.image_loss_restated(img.double(), ref.double(), kind))
    print(f"\n{kind}: {got:.9e} restated in float64 {want:.9e}")
    assert abs(got - want) <= 1e-6 * abs(want)
    assert float(render.image_loss(ref, ref, kind)) == 0.0


def test_color_loss_and_shading_normal_match_their_restatements():
    from meshdiffusion_amd import render
    gen = torch.Generator().manual_seed(12)
    sh, sh2, img, img2 = (torch.rand(2, 6, 5, 4, generator=gen) for _ in range(4))
    for kind in ic.LOSS_KINDS:
        got = float(render.color_loss({"shaded": sh, "shaded_second": sh2}, {"img": img, "img_second": img2}, kind))
        want = float(ic.color_loss_restated(sh.double(), sh2.double(), img.double(), img2.double(), kind))
        assert abs(got - want) <= 1e-6 * abs(want), kind
    # default kind and the layer weights
    a = render.color_loss({"shaded": sh, "shaded_second": img2}, {"img": img, "img_second": img2})
    assert abs(float(a) - float(render.image_loss(sh[..., :3] * img[..., 3:], img[..., :3] * img[..., 3:], "logl1"))) <= 1e-7
    pos, geo = (torch.randn(2, 6, 5, 3, generator=gen) for _ in range(2))
    geo = geo / geo.norm(dim=-1, keepdim=True)
    campos = torch.randn(2, 3, generator=gen) * 3
    nrm = _grazing_normals(pos, campos, gen, torch.float32)
    got = render.shading_normal(pos, campos, nrm, geo)
    want, _, gv, t_raw = ic.shading_normal_restated(pos, campos, nrm, geo, torch.float64)
    safe = (gv.abs() > 1e-4)[..., 0]                                    # the flip cannot differ between fp32 and float64 there
    err = rc.rel_l2(got[safe], want[safe])
    print(f"\nshading_normal: rel-L2 vs float64 {err:.2e} over {int(safe.sum())} of {safe.numel()} pixels; flipped "
          f"{int((gv <= 0).sum())}, bend active {int(((t_raw > 0) & (t_raw < 1)).sum())}")
    assert err <= 1e-5 and int((gv <= 0).sum()) > 0 and int(((t_raw > 0) & (t_raw < 1)).sum()) > 0
    assert float(got.norm(dim=-1).max()) <= 1 + 1e-5
    assert not bool(render.shading_normal(pos, campos, torch.zeros_like(nrm), torch.zeros_like(geo)).any())


def _grazing_normals(pos, campos, gen, dtype):
    """Smooth normals nearly perpendicular to the view vector, so that many pixels sit inside the bend (0 < t < 1)."""
    view = campos.to(dtype)[:, None, None, :] - pos
    view = view / view.norm(dim=-1, keepdim=True)
    r = torch.randn(pos.shape, generator=gen, dtype=dtype)
    perp = r - (r * view).sum(-1, keepdim=True) * view
    c = torch.rand(pos.shape[:-1] + (1,), generator=gen, dtype=dtype) * 0.2 - 0.1
    return perp / perp.norm(dim=-1, keepdim=True) + c * view


def _fd(fn, x, direction, h=1e-6):
    return (float(fn(x + h * direction)) - float(fn(x - h * direction))) / (2 * h)


@pytest.mark.parametrize("case", SMALL, ids=ic.case_id)
def test_central_differences_match_the_autograd_of_the_restatements(case):
    """float64 on the small meshes: interpolate (attr, u, v), the barycentric path, vertex normals, shading normal; 1e-6 relative."""
    verts, faces, mvp, campos, pc, H, W = ic.case_inputs(case)
    rast = ac.rast_restated(pc, faces, H, W)[0]
    B, V, F = pc.shape[0], verts.shape[0], faces.shape[0]
    gen = torch.Generator().manual_seed(21)
    attr = ic.case_attr(V, 3, B, 5).double()
    G = ic.case_G((B, H, W, 3), 6).double()
    _, da, dr = ic.interpolate_grads_restated(attr, rast, faces, G, torch.float64)
    d_attr = torch.randn(attr.shape, generator=gen, dtype=torch.float64)
    d_uv = torch.randn(B, H, W, 2, generator=gen, dtype=torch.float64)
    u0, v0 = rast[..., 0].double(), rast[..., 1].double()
    checks = [("attr", _fd(lambda a: (ic.interpolate_restated(a, rast, faces, torch.float64) * G).sum(), attr, d_attr), float((da * d_attr).sum())),
              ("rast", _fd(lambda s: (ic.interpolate_restated(attr, rast, faces, torch.float64, (u0 + s * d_uv[..., 0], v0 + s * d_uv[..., 1])) * G).sum(),
                           torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)), float((dr[..., :2] * d_uv).sum()))]
    G4 = ic.case_G((B, H, W, 4), 7).double()
    dp = ic.bary_grad_restated(pc, faces, rast, G4, torch.float64)
    d_pc = torch.randn(pc.shape, generator=gen, dtype=torch.float64)

    def bary_value(p):
        u, v = ic.layer_uv(p, faces, rast, torch.float64)
        return (u * G4[..., 0] + v * G4[..., 1]).sum()
    checks.append(("bary", _fd(bary_value, pc.double(), d_pc, 1e-7), float((dp * d_pc).sum())))
    assert not bool(dp[..., 2].any())
    Gn = ic.case_G(verts.shape, 8).double()
    _, dv = ic.vertex_normals_grads_restated(verts, faces, Gn, torch.float64)
    d_v = torch.randn(verts.shape, generator=gen, dtype=torch.float64)
    checks.append(("normals", _fd(lambda x: (ic.vertex_normals_restated(x, faces, torch.float64)[0] * Gn).sum(), verts.double(), d_v), float((dv * d_v).sum())))
    pos, geo = (torch.randn(2, 5, 5, 3, generator=gen, dtype=torch.float64) for _ in range(2))
    geo = geo / geo.norm(dim=-1, keepdim=True)
    nrm = _grazing_normals(pos, campos, gen, torch.float64)
    Gs = torch.randn(2, 5, 5, 3, generator=gen, dtype=torch.float64)
    _, _, gv, t_raw = ic.shading_normal_restated(pos, campos, nrm, geo)
    away = ((t_raw.abs() > 1e-3) & ((t_raw - 1).abs() > 1e-3) & (gv.abs() > 1e-3)).to(torch.float64)
    x = torch.cat([pos, nrm, geo], -1).requires_grad_(True)

    def shade_value(y):
        return (ic.shading_normal_restated(y[..., 0:3], campos, y[..., 3:6], y[..., 6:9])[0] * Gs * away).sum()
    shade_value(x).backward()
    d_x = torch.randn(x.shape, generator=gen, dtype=torch.float64)
    checks.append(("shading", _fd(shade_value, x.detach(), d_x, 1e-7), float((x.grad * d_x).sum())))
    assert int(((t_raw > 0) & (t_raw < 1)).sum()) > 0
    for name, fd, an in checks:
        print(f"\n{ic.case_id(case)} {name}: central differences {fd:.10e} autograd {an:.10e}")
        assert abs(fd - an) <= 1e-6 * abs(an), name


@pytest.mark.parametrize("case", SMALL, ids=ic.case_id)
def test_face_constant_attribute_and_the_mask(case):
    verts, faces, mvp, campos, pc, H, W = ic.case_inputs(case)
    rast = ac.rast_restated(pc, faces, H, W)[0]
    B, F = pc.shape[0], faces.shape[0]
    cov = ic.covered(rast, F)
    assert int(cov.sum()) > 0
    attr = ic.case_attr(F, 3, 1, 3)
    G = ic.case_G((B, H, W, 3), 4)
    for dtype in (torch.float32, torch.float64):
        out, da, dr = ic.interpolate_grads_restated(attr, rast, ic.fff(F), G, dtype)
        want = attr[0].to(dtype)[(rast[..., 3].long() - 1).clamp_min(0)] * cov[..., None]
        assert float((out - want).abs().max()) <= (1e-6 if dtype == torch.float32 else 1e-15)
        assert not bool(dr.any())                                       # A0 = A1 = A2: du = dv = 0 exactly
        ones = ic.interpolate_restated(torch.ones(verts.shape[0], 1), rast, faces, dtype)
        assert float((ones[..., 0] - cov.to(dtype)).abs().max()) <= (1e-6 if dtype == torch.float32 else 1e-15)
    # an id above F is not covered and never an index
    r = rast.clone()
    r[..., 3] = r[..., 3] + F
    assert not bool(ic.interpolate_restated(attr, r, ic.fff(F), torch.float32)[cov].any())


def test_vertex_normals_of_the_degenerate_mesh():
    verts, faces = ic.mesh("degen")
    n, fn, replaced = ic.vertex_normals_restated(verts, faces, torch.float64)
    assert replaced.tolist() == [False] * 4 + [True] * 4
    assert torch.equal(n[4:], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(4, 3)) and not bool(fn[2:].any())
    _, g = ic.vertex_normals_grads_restated(verts, faces, ic.case_G(verts.shape, 1), torch.float64)
    assert not bool(g[4:].any()) and bool(g[:4].any())
    fv, ff = ic.mesh("fan40")
    assert int((ff == 0).sum()) == ic.FAN and ff.shape == (ic.FAN, 3)


def test_fixture_is_small_and_holds_every_unit(gold):
    assert os.path.getsize(os.path.join(GOLD, "interp.npz")) < 256 * 1024
    assert all(gold[k].size <= 4 for k in gold.files)                   # seeds and scalars, no images
    for case in ic.CASES:
        cid = ic.case_id(case)
        verts, faces = ic.mesh(case[0])
        for layer in (0, 1):
            for name, *_ in ic.attr_cases(verts.shape[0], faces.shape[0], faces, 2):
                for q in ("value", "dattr", "drast"):
                    assert 0 <= float(gold[f"case/{cid}/L{layer}/{name}/ref_err_{q}"]) < 1e-5, (cid, layer, name, q)
            assert 0 <= float(gold[f"case/{cid}/L{layer}/ref_err_dpos"]) < 1e-3 and 0 <= float(gold[f"case/{cid}/L{layer}/ref_err_depth"]) < 1e-5
        assert 0 < float(gold[f"case/{cid}/ref_err_chain_dverts"]) < 1e-3
        assert 0 < float(gold[f"normals/{case[0]}/ref_err_dverts"]) < 1e-5
    for case in ic.BUFFER_CASES:
        cid = ic.case_id(case)
        assert 0 < float(gold[f"buffers/{cid}/ref_err_dverts"]) < 1e-3
        assert (gold[f"buffers/{cid}/min_geo_view"] >= ic.FLIP_MARGIN).all()
    assert tuple(gold["fit/steps"]) == ic.FIT_STEPS
    for k in ("depth", "alpha", "color"):
        for p in ("32", "64"):
            assert gold[f"fit/{k}{p}"].shape == (3,) and np.isfinite(gold[f"fit/{k}{p}"]).all()
