"""Host side of the fixed-topology second pass (csrc/fixedtopo.hip, meshdiffusion_amd/dmtet.py, meshdiffusion_amd/render.py)
without a GPU: the export tables, argument refusal, and the restatements of tests/fixedtopo_cases.py against themselves -- central
differences against their autograd, a flat patch, the sign of zero, the depth term's blind layer, the schedule."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fixedtopo_cases as fc
from conftest import GOLD, ROOT


def test_new_exports_are_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import _lib, build, dmtet, render
    header = open(os.path.join(ROOT, "include", "meshdiffusion_hip.h")).read()
    assert "fixedtopo.hip" in build.SOURCES
    assert _lib.LAPLACE_WORKSPACE_BYTES == 512 and "#define MD_LAPLACE_SLABS 64" in header
    src = open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "fixedtopo.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "THE FIXED-TOPOLOGY CONTRACT" in src and "atomicAdd" not in src
    for name in ("laplace_regularizer_const", "depth_loss_fixedtopo", "fit_fixed_topology", "lr_schedule_fixedtopo"):
        assert callable(getattr(render, name)), name
    for name in ("FixedTopoPlan", "DMTetGeometryFixedTopo", "face_corner_csr", "fixed_sign"):
        assert callable(getattr(dmtet, name)), name


def test_new_exports_refuse_bad_arguments_without_a_gpu(hip_lib):
    nul, one, odd8, odd4 = C.c_void_p(0), C.c_void_p(64), C.c_void_p(68), C.c_void_p(66)

    def check(fn, ok, pointers, sizes, unsupported, misaligned, optional=()):
        for k in pointers:
            a = list(ok); a[k] = nul
            assert fn(*a) == -1, (fn.__name__, k)
        for k in optional:
            a = list(ok); a[k] = odd4
            assert fn(*a) == -1, (fn.__name__, k)
        for k in sizes:
            for bad in (0, -3):
                a = list(ok); a[k] = bad
                assert fn(*a) == -1, (fn.__name__, k, bad)
        for k, v in unsupported:
            a = list(ok); a[k] = v
            assert fn(*a) == -2, (fn.__name__, k, v)
        for k, p in misaligned:
            a = list(ok); a[k] = p
            assert fn(*a) == -1, (fn.__name__, k)

    # md_fixedtopo_verts(pos, sdf, edge, N, Vm, verts, stream)
    check(hip_lib.md_fixedtopo_verts, [one, one, one, 1000, 300, one, nul], (0, 1, 2, 5), (3, 4),
          ((3, 1 << 31), (4, 1 << 30), (3, 1 << 40)), ((0, odd4), (1, odd4), (2, odd8), (5, odd4)))
    # md_fixedtopo_verts_bwd(g, sdf, edge, ptr, inc, N, Vm, dpos, stream)
    check(hip_lib.md_fixedtopo_verts_bwd, [one, one, one, one, one, 1000, 300, one, nul], (0, 1, 2, 3, 4, 7), (5, 6),
          ((5, 1 << 31), (6, 1 << 30)), ((0, odd4), (2, odd8), (3, odd4), (4, odd4), (7, odd4)))
    # md_laplace_umbrella(x, base, faces, ptr, order, V, F, term, workspace, loss, stream); base may be null
    ok = [one, one, one, one, one, 100, 300, one, one, one, nul]
    check(hip_lib.md_laplace_umbrella, ok, (0, 2, 3, 4, 7, 8, 9), (5, 6), ((5, 1 << 31), (6, 1 << 24), (6, 1 << 33)),
          ((0, odd4), (2, odd8), (3, odd4), (4, odd4), (7, odd4), (8, odd8), (9, odd4)), optional=(1,))
    # md_laplace_umbrella_bwd(term, faces, ptr, order, grad_out, V, F, q, dx, stream)
    ok = [one, one, one, one, one, 100, 300, one, one, nul]
    check(hip_lib.md_laplace_umbrella_bwd, ok, (0, 1, 2, 3, 4, 7, 8), (5, 6), ((5, 1 << 31), (6, 1 << 24)),
          ((0, odd4), (1, odd8), (2, odd4), (3, odd4), (4, odd4), (7, odd4), (8, odd4)))


def test_python_entry_points_refuse_cpu_tensors_and_bad_shapes(monkeypatch):
    from meshdiffusion_amd import _lib, dmtet, render
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [0, 2, 3]])
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.laplace_regularizer_const(v, f)                          # CPU tensors: no fallback
    with pytest.raises(_lib.MeshDiffusionHipError):
        dmtet.FixedTopoPlan(None, torch.zeros(5, 3), torch.zeros(5))
    with pytest.raises(_lib.MeshDiffusionHipError):
        dmtet.DMTetGeometryFixedTopo(type("G", (), {"sdf": torch.nn.Parameter(torch.zeros(5))})(), 64, 2.1)
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.fit_fixed_topology(type("G", (), {"deform": torch.zeros(5, 3)})(), {}, 1)
    monkeypatch.setattr(render, "_gpu_only", lambda t, what: None)      # the shape checks come before any launch
    for bad_v, bad_f, base in ((torch.zeros(4), f, None), (torch.zeros(0, 3), f, None), (v, torch.tensor([[0, 1]]), None),
                               (v, torch.zeros(0, 3, dtype=torch.int64), None), (v, f, torch.zeros(3, 3)), (v, torch.tensor([[0, 1, 4]]), None)):
        with pytest.raises(ValueError):
            render.laplace_regularizer_const(bad_v, bad_f, base=base)
    with pytest.raises(ValueError):
        render.laplace_regularizer_const(v, f, corner_csr=(torch.zeros(4, dtype=torch.int32), torch.zeros(6, dtype=torch.int32)))
    ptr, order = dmtet.face_corner_csr(f, 4)
    assert ptr.tolist() == [0, 2, 3, 5, 6] and order.tolist() == [0, 3, 1, 2, 4, 5] and ptr.dtype == order.dtype == torch.int32


def _fd(fn, x, direction, h=1e-6):
    return (float(fn(x + h * direction)) - float(fn(x - h * direction))) / (2 * h)


def test_vertex_formula_on_the_two_tet_grid():
    pos, tets = fc.two_tet_grid()
    edges = fc.sorted_edges(tets)
    assert edges.shape == (9, 2)                                        # 6 + 6 - the 3 of the shared face
    gen = torch.Generator().manual_seed(3)
    for sdf in (torch.tensor([1.0, -1.0, -1.0, 1.0, -1.0]), torch.tensor([0.3, -0.9, 0.2, 0.7, -0.4])):
        sdf = sdf.double()
        edge = fc.crossing_edges(sdf, edges)
        assert 0 < edge.shape[0] < 9 and bool((edge[:, 0] < edge[:, 1]).all())
        G = torch.randn(edge.shape[0], 3, generator=gen, dtype=torch.float64)
        p = pos.clone().requires_grad_(True)
        v = fc.verts_restated(p, sdf, edge)
        (v * G).sum().backward()
        if bool((sdf.abs() == 1).all()):
            assert torch.equal(v.detach(), 0.5 * pos[edge[:, 0]] + 0.5 * pos[edge[:, 1]])       # +-1: the exact midpoint
        d = torch.randn(pos.shape, generator=gen, dtype=torch.float64)
        fd, an = _fd(lambda x: (fc.verts_restated(x, sdf, edge) * G).sum(), pos, d), float((p.grad * d).sum())
        print(f"\ntwo tets, sdf {sdf.tolist()}: Vm {edge.shape[0]} central differences {fd:.10e} autograd {an:.10e}")
        assert abs(fd - an) <= 1e-6 * abs(an)
        # the gradient of grid vertex n is the sum of g[i] * weight over the codes of n: the gather of the contract
        w0, w1 = -sdf[edge[:, 1]] / (sdf[edge[:, 0]] - sdf[edge[:, 1]]), sdf[edge[:, 0]] / (sdf[edge[:, 0]] - sdf[edge[:, 1]])
        want = torch.zeros_like(pos).index_add(0, edge[:, 0], G * w0[:, None]).index_add(0, edge[:, 1], G * w1[:, None])
        assert float((p.grad - want).abs().max()) <= 1e-15


@pytest.mark.parametrize("name", fc.SMALL_MESHES)
@pytest.mark.parametrize("kind", fc.BASES)
def test_laplacian_central_differences_match_autograd(name, kind):
    x, base, faces = fc.laplace_case(name)
    b = base if kind == "base" else None
    val, dx = fc.laplace_grads_restated(x, faces, b, torch.float64, grad_out=1.0)
    d = torch.randn(x.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    fd, an = _fd(lambda y: fc.laplace_restated(y, faces, b)[0], x.double(), d), float((dx * d).sum())
    print(f"\nlaplace {name} {kind}: value {float(val):.6e} central differences {fd:.10e} autograd {an:.10e}")
    assert abs(fd - an) <= 1e-6 * abs(an)
    # the backward of the contract, written as its gather formula
    V = x.shape[0]
    _, term = fc.laplace_restated(x, faces, b)
    corners = torch.bincount(faces.reshape(-1), minlength=V).double()
    q = (2.0 / (3 * V)) * term / torch.clamp(2 * corners, min=1.0)[:, None]
    c = q[faces]
    want = torch.zeros(V, 3, dtype=torch.float64).index_add(0, faces.reshape(-1), ((c[:, [1, 2, 0]] + c[:, [2, 0, 1]]) - 2 * c).reshape(-1, 3))
    assert float((dx - want).abs().max()) <= 1e-12 * float(dx.abs().max())
    if name == "degen":
        assert not bool(term[4:].any()) and not bool(dx[4:].any())       # the vertex no face names; one point three times


def test_laplacian_of_a_flat_regular_patch_and_the_reference_form():
    verts, faces, interior = fc.flat_patch(5)
    val, term = fc.laplace_restated(verts, faces)
    assert int(interior.sum()) == 9 and not bool(term[interior].any()) and bool(term[~interior].any())
    assert float(fc.laplace_restated(verts, faces, base=verts)[0]) == 0.0
    for name in fc.SMALL_MESHES:                                        # the restatement is the reference's scatter_add form
        x, base, f = fc.laplace_case(name)
        a, b = float(fc.laplace_restated(x - base, f, None, torch.float64)[0]), float(fc.laplace_reference((x - base).double(), f))
        assert abs(a - b) <= 1e-12 * abs(b), name


def test_the_sign_of_zero_is_plus_one():
    from meshdiffusion_amd.dmtet import fixed_sign
    s = fixed_sign(torch.tensor([0.0, -0.0, 1e-9, -1e-9, -1e-8, -0.5, 2.0, -1e-3]))
    assert s.tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0] and s.dtype == torch.float32


def test_depth_loss_fixedtopo_ignores_layer_one():
    from meshdiffusion_amd import render
    gen = torch.Generator().manual_seed(7)
    B, H, W = 2, 6, 5
    t1 = torch.rand(B, H, W, 1, generator=gen) + 2
    t2 = t1 + torch.rand(B, H, W, 1, generator=gen) * 0.02                # some pairs closer than 5e-3, some not
    t2[0, 0, :2] = -1.0                                                  # no second layer there
    mask = (torch.rand(B, H, W, 1, generator=gen) > 0.3).float()
    tgt = {"depth": t1, "depth_second": t2, "mask_cont": mask}
    d2 = t2 + torch.randn(B, H, W, 1, generator=gen) * 8                  # both sides of the Huber threshold after the 0.1
    buf = {"depth": torch.rand(B, H, W, 1, generator=gen), "depth_second": d2}
    a = render.depth_loss_fixedtopo(buf, tgt)
    b = render.depth_loss_fixedtopo({"depth": buf["depth"] + 5.0, "depth_second": d2}, tgt)
    assert torch.equal(a, b) and float(a) > 0                            # layer 1 does not enter
    c = render.depth_loss_fixedtopo({"depth": buf["depth"], "depth_second": d2 + 1.0}, tgt)
    assert not torch.equal(a, c)
    want = fc.depth_loss_fixedtopo_restated(d2.double(), t1.double(), t2.double(), mask[..., 0].double())
    prox = ((t2 - t1).abs() >= 5e-3)
    print(f"\ndepth_loss_fixedtopo {float(a):.9e} restated in float64 {float(want):.9e}; pairs under 5e-3: {int((~prox).sum())}, "
          f"quadratic pixels {int((((d2 - t2).abs() * 0.1) >= 1).sum())}")
    assert abs(float(a) - float(want)) <= 1e-6 * abs(float(want))
    assert 0 < int((~prox).sum()) < prox.numel() and int((((d2 - t2).abs() * 0.1) >= 1).sum()) > 0
    buf["depth_second"].requires_grad_(True)
    buf["depth"].requires_grad_(True)
    render.depth_loss_fixedtopo(buf, tgt).backward()
    assert buf["depth"].grad is None and bool(buf["depth_second"].grad.any())


def test_learning_rate_schedule():
    from meshdiffusion_amd import render
    for it, want in ((0, 0.0), (50, 0.5), (100, 1.0), (5100, 0.1)):
        got = render.lr_schedule_fixedtopo(it)
        assert abs(got - want) <= 1e-12 and abs(fc.lr_schedule_restated(it) - want) <= 1e-12, (it, got)
    assert render.lr_schedule_fixedtopo(5, warmup_iter=10) == 0.5
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=render.lr_schedule_fixedtopo)
    assert opt.param_groups[0]["lr"] == 0.0                              # the first step of pass 2 moves nothing


def test_fixture_is_small_and_holds_every_unit():
    gold = np.load(os.path.join(GOLD, "fixedtopo.npz"))
    assert os.path.getsize(os.path.join(GOLD, "fixedtopo.npz")) < 64 * 1024
    assert all(gold[k].size == 1 for k in gold.files)                    # seeds and scalars only
    assert int(gold["laplace/x_seed"]) == fc.X_SEED and float(gold["laplace/grad_out"]) == fc.GRAD_OUT
    for name in fc.LAPLACE_MESHES:
        for kind in fc.BASES:
            assert fc.HALF_ULP <= float(gold[f"laplace/{name}/{kind}/ref_err_value"]) < 1e-6
            assert 0 < float(gold[f"laplace/{name}/{kind}/ref_err_dx"]) < 1e-6
