"""Host side of the silhouette antialiasing (meshdiffusion_amd/render.py, csrc/antialias.hip) without a GPU: the export tables,
argument refusal, and the restatement of the antialiasing contract in tests/antialias_cases.py itself -- exact sums on a
rectangle, central differences against its autograd, an image without candidate pairs, one edge per pair, the edge neighbours
of hand-made meshes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import antialias_cases as ac
from conftest import GOLD, ROOT


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "antialias.npz"))


def _nbr(faces, n_verts):
    return torch.as_tensor(ac.edge_neighbours_restated(faces.numpy(), n_verts))


def test_new_exports_are_declared_everywhere_and_abi_stays_16(hip_lib):
    from meshdiffusion_amd import build, render
    assert "antialias.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "antialias.hip")).read()
    assert "#pragma clang fp contract(off)" in src and '#include "md_raster_snap.h"' in src and "rs_snap(float" not in src
    assert '#include "md_raster_snap.h"' in open(os.path.join(ROOT, "meshdiffusion_amd", "csrc", "raster.hip")).read()
    for name in ("edge_neighbours", "antialias", "silhouette_loss"):
        assert callable(getattr(render, name)), name


def test_new_exports_refuse_bad_arguments_without_a_gpu(hip_lib):
    nul, one, odd = C.c_void_p(0), C.c_void_p(64), C.c_void_p(68)

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

    # md_mesh_edge_neighbours(sorted_keys, order, faces, F, nbr, stream)
    ok = [one, one, one, 300, one, nul]
    refuses(hip_lib.md_mesh_edge_neighbours, ok, (0, 1, 2, 4), (3,))
    unsupported(hip_lib.md_mesh_edge_neighbours, ok, ((3, 1 << 24),))
    # md_antialias_pairs(rast, pos_clip, faces, nbr, B, V, F, H, W, pairs, stream)
    ok = [one, one, one, one, 2, 100, 300, 64, 48, one, nul]
    refuses(hip_lib.md_antialias_pairs, ok, (0, 1, 2, 3, 9), (4, 5, 6, 7, 8))
    unsupported(hip_lib.md_antialias_pairs, ok, ((4, 65), (6, 1 << 24), (7, 2049), (8, 2049)))
    for k in (0, 1, 9):                                               # 16-byte loads and stores
        a = list(ok); a[k] = odd
        assert hip_lib.md_antialias_pairs(*a) == -1, k
    # md_antialias_blend(color, pairs, B, H, W, C, out, stream) and md_antialias_bwd_color(grad_out, pairs, B, H, W, C, dcolor, stream)
    for fn in (hip_lib.md_antialias_blend, hip_lib.md_antialias_bwd_color):
        ok = [one, one, 2, 64, 48, 3, one, nul]
        refuses(fn, ok, (0, 1, 6), (2, 3, 4))
        unsupported(fn, ok, ((2, 65), (3, 2049), (4, 2049), (5, 0), (5, 9), (5, -1)))
        a = list(ok); a[1] = odd
        assert fn(*a) == -1
    # md_antialias_bwd_pos(active, n_active, color, grad_out, pairs, pos_clip, ptr, order, B, V, H, W, C, vert_grad, dpos_clip, stream)
    ok = [one, 500, one, one, one, one, one, one, 2, 100, 64, 48, 3, one, one, nul]
    refuses(hip_lib.md_antialias_bwd_pos, ok, (0, 2, 3, 4, 5, 6, 7, 13, 14), (8, 9, 10, 11))
    unsupported(hip_lib.md_antialias_bwd_pos, ok, ((8, 65), (10, 2049), (11, 2049), (12, 0), (12, 9)))
    a = list(ok); a[1] = -1
    assert hip_lib.md_antialias_bwd_pos(*a) == -1
    a = list(ok); a[1] = (1 << 30) + 1
    assert hip_lib.md_antialias_bwd_pos(*a) == -2                     # 2 n_active must fit the int32 codes
    a = list(ok); a[8], a[9] = 64, 1 << 26
    assert hip_lib.md_antialias_bwd_pos(*a) == -2                     # B V must fit the int32 CSR


def test_host_functions_check_their_arguments():
    from meshdiffusion_amd import _lib, render
    col, rast, pc, f = torch.zeros(1, 8, 8, 1), torch.zeros(1, 8, 8, 4), torch.zeros(1, 4, 4), torch.tensor([[0, 1, 2]])
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.antialias(col, rast, pc, f)                              # CPU tensor: no fallback
    with pytest.raises(_lib.MeshDiffusionHipError):
        render.edge_neighbours(f, 4)
    a = torch.rand(2, 5, 5, 1)
    got = render.silhouette_loss({"alpha": a, "alpha_second": a * 0.5}, {"alpha": a * 0.0, "alpha_second": a})
    want = ac.silhouette_loss_restated(a.double(), a.double() * 0.5, a.double() * 0.0, a.double())
    assert abs(float(got) - float(want)) <= 1e-6 * float(want)


def test_rectangle_gives_exact_row_and_column_sums():
    """The mask of a rectangle with edges at 2.3 .. 11.7 x 3.6 .. 12.2 pixels: antialiased rows sum to its width, columns to its
    height (fp32, 1e-6 absolute), away from the corners."""
    pc, faces = ac.small_mesh("quad")
    x0, x1, y0, y1 = ac.RECT
    rast, _ = ac.rast_restated(pc, faces, 16, 16)
    mask = (rast[..., 3] > 0).float()[..., None]
    assert int(mask.sum()) == 10 * 8                                    # columns 2 .. 11, rows 4 .. 11
    out = ac.antialias_restated(mask, rast, pc, faces, _nbr(faces, 4), torch.float32)[0, :, :, 0]
    assert out.dtype == torch.float32
    rows, cols = out.sum(1)[5:11], out.sum(0)[3:11]
    print(f"\nrectangle: row sums {rows.tolist()} column sums {cols.tolist()}")
    assert float((rows - (x1 - x0)).abs().max()) <= 1e-6 and float((cols - (y1 - y0)).abs().max()) <= 1e-6
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    # the diagonal is shared by the two triangles and lies inside the silhouette: no pair on it is active
    dec = ac.pair_decisions(rast, pc, faces, _nbr(faces, 4))
    inner = torch.zeros(16, 16, dtype=torch.bool)
    inner[4:11, 2:11] = True
    assert not bool(dec["active"][0][inner].any()) and int(dec["active"].sum()) >= 2 * (10 + 8) - 4


def test_central_differences_match_the_autograd_of_the_restatement():
    """float64, the parametric torus at 64 x 64: d sum(G * out) / d pos_clip along a random direction, 1e-6 relative."""
    case = ac.CASES[1]
    pc, faces, H, W = ac.case_inputs(case)
    nbr = _nbr(faces, pc.shape[1])
    rast, _ = ac.rast_restated(pc, faces, H, W)
    dec = ac.pair_decisions(rast, pc, faces, nbr)
    col = ac.case_colour("c3", rast[..., 3] > 0, 5)
    G = ac.case_G(col.shape, 6)
    _, dcol, dpos = ac.grads_restated(col, rast, pc, faces, nbr, G, torch.float64, dec)
    gen = torch.Generator().manual_seed(7)
    dirp = torch.randn(pc.shape, generator=gen, dtype=torch.float64)
    dirc = torch.randn(col.shape, generator=gen, dtype=torch.float64)

    def value(p, c):
        return float((ac.antialias_restated(c, rast, p, faces, nbr, torch.float64, dec) * G.double()).sum())
    h = 1e-6
    fd_p = (value(pc.double() + h * dirp, col.double()) - value(pc.double() - h * dirp, col.double())) / (2 * h)
    fd_c = (value(pc.double(), col.double() + h * dirc) - value(pc.double(), col.double() - h * dirc)) / (2 * h)
    an_p, an_c = float((dpos * dirp).sum()), float((dcol * dirc).sum())
    print(f"\ncentral differences / autograd: pos_clip {fd_p:.10e} / {an_p:.10e}  color {fd_c:.10e} / {an_c:.10e}")
    assert abs(fd_p - an_p) <= 1e-6 * abs(an_p) and abs(fd_c - an_c) <= 1e-6 * abs(an_c)
    assert not bool(dpos[..., 2].any())                                 # no z component
    on_edge = torch.zeros(pc.shape[:2], dtype=torch.bool)
    b = torch.nonzero(dec["active"])[:, 0]
    on_edge[b, dec["va"][dec["active"]]] = True
    on_edge[b, dec["vb"][dec["active"]]] = True
    assert not bool(dpos[~on_edge].any()) and bool((~on_edge).any()) and bool(on_edge.any())


def test_image_without_candidate_pairs_comes_back_bit_equal():
    pc, faces, H, W = ac.case_inputs(ac.CASES[1])
    nbr = _nbr(faces, pc.shape[1])
    col = torch.rand(2, H, W, 3, generator=torch.Generator().manual_seed(1))
    for ident in (0.0, 7.0):                                            # nothing covered; one triangle everywhere
        rast = torch.zeros(2, H, W, 4)
        rast[..., 3] = ident
        rast[..., 2] = torch.rand(2, H, W, generator=torch.Generator().manual_seed(2))
        dec = ac.pair_decisions(rast, pc, faces, nbr)
        assert not bool(dec["active"].any())
        assert torch.equal(ac.antialias_restated(col, rast, pc, faces, nbr, torch.float32, dec), col)
    # ids above F take no part
    rast[..., 3] = torch.randint(faces.shape[0] + 1, faces.shape[0] + 50, (2, H, W), generator=torch.Generator().manual_seed(3)).float()
    assert not bool(ac.pair_decisions(rast, pc, faces, nbr)["active"].any())


@pytest.mark.parametrize("case", ac.CASES[:5], ids=ac.case_id)
def test_a_pair_is_never_given_two_edges(case, gold):
    pc, faces, H, W = ac.case_inputs(case)
    nbr = _nbr(faces, pc.shape[1])
    for layer, rast in enumerate(ac.rast_restated(pc, faces, H, W)):
        dec = ac.pair_decisions(rast, pc, faces, nbr)
        n = int(dec["active"].sum())
        print(f"\n{ac.case_id(case)} layer {layer}: active pairs {n}, most edges passing in one pair {int(dec['n_pass'].max())}")
        assert int(dec["n_pass"].max()) <= 1
        assert bool((dec["active"] <= (dec["n_pass"] == 1)).all())
        assert bool(((dec["va"] >= 0) == dec["active"]).all()) and bool(((dec["vb"] >= 0) == dec["active"]).all())
        assert n == int(gold[f"case/{ac.case_id(case)}/L{layer}/active"])
        assert not bool(dec["active"][:, :, -1, 0].any()) and not bool(dec["active"][:, -1, :, 1].any())
    assert int(gold[f"case/{ac.case_id(case)}/L0/active"]) > 0


def test_edge_neighbours_of_hand_made_meshes():
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    nbr = ac.edge_neighbours_restated(tet, 4)
    assert (nbr >= 0).all() and all(nbr[f, k] not in tet[f] for f in range(4) for k in range(3))
    quad = np.array([[0, 1, 2], [0, 2, 3]])
    nbr = ac.edge_neighbours_restated(quad, 4)
    assert int((nbr < 0).sum()) == 4 and nbr[0, 1] == 3 and nbr[1, 2] == 1          # the diagonal 0-2
    fan = ac.small_mesh("fan3")[1].numpy()
    nbr = ac.edge_neighbours_restated(fan, 5)
    assert (nbr < 0).all() and all((nbr[f, list(fan[f]).index(v)] == -1) for f in range(3) for v in fan[f] if v >= 2)
    tv, tf = ac.param_torus()
    nbr = ac.edge_neighbours_restated(tf.numpy(), tv.shape[0])
    assert nbr.shape == (2 * ac.TORUS_NU * ac.TORUS_NV, 3) and (nbr >= 0).all()
    f = tf.numpy()
    for fi in (0, 17, 255):                                             # the neighbour vertex forms a face with the edge
        for k in range(3):
            want = {int(f[fi, (k + 1) % 3]), int(f[fi, (k + 2) % 3]), int(nbr[fi, k])}
            assert any(set(map(int, row)) == want for row in f), (fi, k)
    assert ac.edge_neighbours_restated(np.zeros((0, 3), np.int64), 3).shape == (0, 3)


def test_fixture_is_small_and_holds_every_unit(gold):
    assert os.path.getsize(os.path.join(GOLD, "antialias.npz")) < 64 * 1024
    for case in ac.CASES:
        for layer in (0, 1):
            for kind in ac.COLOURS:
                for q in ("value", "dcolor", "dpos"):
                    assert 0 <= float(gold[f"case/{ac.case_id(case)}/L{layer}/{kind}/ref_err_{q}"]) < 1e-5, (case, layer, kind, q)
    assert tuple(gold["fit/steps"]) == ac.FIT_STEPS
    for k in ("depth32", "depth64", "alpha32", "alpha64"):
        assert gold[f"fit/{k}"].shape == (3,) and np.isfinite(gold[f"fit/{k}"]).all()
    assert gold["fit/iou_small_start"].shape == (2,) and 0 < float(gold[f"alpha/{ac.case_id(ac.CASES[1])}/ref_err_dverts"]) < 1e-5
