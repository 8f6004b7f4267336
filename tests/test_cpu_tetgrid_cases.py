"""The cases of tests/test_gpu_tetgrid.py, proven without a GPU (tests/tetgrid_cases.py holds them).

Every case is shown to be in the regime its name claims; a numpy emulation of the KERNEL's formulation of marching tetrahedra
(static edge table, chunk totals, scan in passes with a carry, prefix ids) equals the oracle's run-time sort-and-unique algorithm on
every case; and one-line mutations of that emulation -- the mistakes such a kernel makes -- differ from the oracle on the case
that owns the path.  So the GPU test can fail, and a case that no mutation can fail is not a case.  The host tables
(`TetTables`, `build_incidence`, `GridMesher.inputs`) are pure torch and are checked here against loops and numpy.
"""
import numpy as np
import pytest
import torch

import tetgrid_cases as tc
from oracle import dmtet_oracle

# name: (N, T, E, edge chunks, tet chunks)
SIZES = {"one-tet": (4, 1, 6, 1, 1), "T1023": (343, 1023, None, 2, 1), "T1024": (343, 1024, None, 2, 1),
         "T1025": (343, 1025, None, 2, 2), "E1023": (343, 242, 1023, 1, 1), "E1024": (343, 244, 1024, 1, 1),
         "E1025": (343, 238, 1025, 2, 1), "N255": (255, 900, 1321, 2, 1), "N256": (256, 900, 1321, 2, 1),
         "N257": (257, 900, 1321, 2, 1), "star": (3004, 3000, 9003, 9, 3), "two-pass": (185193, 1053696, 1257704, 1229, 1029)}


def _oracle(c, sdf):
    with np.errstate(all="ignore"):                      # FLT_MAX - (-FLT_MAX) overflows on purpose
        return dmtet_oracle.marching_tets(c.pos.numpy(), np.asarray(sdf, np.float32), c.tets)


def _crossing(c, sdf):
    edges = tc.case_tables(c.name)[0]
    occ = np.asarray(sdf, np.float32) > 0
    return occ[edges[:, 0]] != occ[edges[:, 1]]


# ---------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------
def _signed_volumes(verts, tets):
    p = verts.astype(np.float64)[tets.astype(np.int64)]
    return np.linalg.det(np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]], 1)) / 6


def test_kuhn_is_the_freudenthal_split():
    nx, ny, nz = 2, 3, 4
    v, t = tc.kuhn(nx, ny, nz)
    assert v.dtype == np.float32 and v.shape == ((nx + 1) * (ny + 1) * (nz + 1), 3) and t.dtype == np.int32 and t.shape == (6 * nx * ny * nz, 4)
    for i, j, k in ((0, 0, 0), (1, 2, 3), (2, 3, 4)):
        assert tuple(v[(i * (ny + 1) + j) * (nz + 1) + k]) == (i, j, k)
    vol = _signed_volumes(v, t)
    assert np.allclose(vol, 1 / 6) and abs(vol.sum() - nx * ny * nz) < 1e-9              # same orientation, and they fill the box
    cells = v[t.astype(np.int64)].min(1).reshape(-1, 6, 3)                                # cell-major: six tets per cell corner
    assert (cells == cells[:, :1]).all() and tuple(cells[1, 0]) == (0, 0, 1) and tuple(cells[nz, 0]) == (0, 1, 0)
    E = tc.edge_table(t, v.shape[0])[0].shape[0]
    assert E == (nx * (ny + 1) * (nz + 1) + (nx + 1) * ny * (nz + 1) + (nx + 1) * (ny + 1) * nz                  # axes
                 + nx * ny * (nz + 1) + nx * (ny + 1) * nz + (nx + 1) * ny * nz + nx * ny * nz)                 # face and body diagonals


def test_rotation_is_even_and_reaches_every_corner_order():
    assert tc.EVEN_PERMS.shape == (12, 4) and len({tuple(p) for p in tc.EVEN_PERMS}) == 12
    v, t = tc.kuhn(3, 3, 3)
    r = tc.rotated(t, 1)
    assert np.array_equal(np.sort(r, 1), np.sort(t, 1)) and not np.array_equal(r, t)
    assert np.allclose(_signed_volumes(v, r), 1 / 6)                                      # an odd permutation would flip the sign
    assert len({tuple(np.argsort(a)[np.argsort(np.argsort(b))]) for a, b in zip(t[:160], r[:160])}) == 12
    # every sign case meets several corner orders on a rotated lattice case
    c = tc.case("N256")
    idx = tc.tet_sign_cases(tc.sdf_randn(c).numpy(), c.tets)
    low = np.argmin(c.tets, 1)                                                            # where the tet's lowest vertex id sits
    assert all(len(set(low[idx == k])) == 4 for k in range(16))


def test_the_recorded_edge_chunk_pairs_are_what_the_search_finds():
    for E, pair in tc.E_CASES.items():
        hits = tc.edge_count_search(E)
        print(f"E = {E}: {hits}")
        assert pair in hits
        grid = tc.truncated(tc.kuhn(6, 6, 6), *pair)
        assert tc.edge_table(grid[1], 343)[0].shape[0] == E
    v, t = tc.truncated(tc.kuhn(6, 6, 6), 3, 40)
    full = tc.kuhn(6, 6, 6)[1]
    assert t.shape == (40, 4) and np.array_equal(t, full[np.random.default_rng(3).permutation(full.shape[0])[:40]])


def test_tables_are_the_kernels():
    assert np.array_equal(tc.TRI_TABLE, dmtet_oracle.TRIANGLE_TABLE) and np.array_equal(tc.NUM_TRI, dmtet_oracle.NUM_TRIANGLES)
    assert tuple(dmtet_oracle.BASE_TET_EDGES) == tc.BASE_TET_EDGES
    with np.errstate(all="ignore"):
        assert np.float32(tc.SUBNORMAL) > 0 and np.float32(tc.SUBNORMAL) / np.float32(2) == 0 and np.isinf(np.float32(tc.FLT_MAX) * np.float32(2))


# ---------------------------------------------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.CASES)
def test_case_is_in_the_regime_its_name_claims(name):
    c = tc.case(name)
    edges, tet_edges = tc.case_tables(name)
    N, T, E, ce, ct = SIZES[name]
    got_ce, got_ct = -(-edges.shape[0] // tc.CHUNK), -(-c.T // tc.CHUNK)
    print(f"{name}: N {c.N} T {c.T} E {edges.shape[0]} edge chunks {got_ce} tet chunks {got_ct} vertex blocks {-(-c.N // tc.BLOCK)}")
    assert (c.N, c.T) == (N, T) and (E is None or edges.shape[0] == E) and (got_ce, got_ct) == (ce, ct)
    assert c.pos.dtype == torch.float32 and c.tets.dtype == np.int32 and c.tets.min() >= 0 and c.tets.max() < c.N
    assert float((c.pos - torch.from_numpy(c.lattice)).abs().max()) <= 0.3 + 1e-6
    assert np.array_equal(edges[tet_edges.reshape(-1)].reshape(-1, 6, 2),
                          np.sort(c.tets.astype(np.int64)[:, list(tc.BASE_TET_EDGES)].reshape(-1, 6, 2), -1))
    deg = np.bincount(edges.reshape(-1), minlength=c.N)
    named = np.setdiff1d(np.arange(c.N), c.unnamed)
    assert (deg[c.unnamed] == 0).all() and (deg[named] > 0).all()                        # empty rows exactly where claimed
    sdf = tc.sdf_randn(c).numpy()
    idx = tc.tet_sign_cases(sdf, c.tets)
    cross = _crossing(c, sdf)
    assert cross.any()                                                                    # a surface: FixedTopoPlan needs one
    if name == "one-tet":
        pat = tc.sign_patterns().numpy()
        assert [int(tc.tet_sign_cases(p, c.tets)[0]) for p in pat] == list(range(16))
        assert c.unnamed.size == 0
    elif name == "star":
        assert deg[0] == tc.STAR_N + 2 >= 3000 and c.unnamed.tolist() == [c.N - 1] and (c.tets[:, 0] == 0).all()
        assert deg[1:-1].max() <= 5                                                       # one long row among short ones
        assert int((cross & (edges[:, 0] == 0)).sum()) >= 1000                            # of which > 1000 codes carry a term
    else:
        assert len(np.unique(idx)) == 16                                                  # every lattice case: all 16 sign cases
    if name[0] in "TEN" or name == "star":
        assert cross[-1] and tc.NUM_TRI[idx[-1]] > 0                                      # the item next to the edge does something
    if name[0] == "N":
        assert c.unnamed.tolist() == list(range(252, c.N)) and -(-c.N // tc.BLOCK) == (2 if c.N > 256 else 1)
    if name[0] == "E":
        assert 0 < c.unnamed.size < c.N // 4 and c.appended == 0                          # empty rows between the others
    if name == "two-pass":
        assert got_ce > tc.CHUNK and got_ct > tc.CHUNK
        vo, fo, fto = _oracle(c, sdf)
        assert vo.shape[0] == int(cross.sum())                                            # the oracle's vertices are these crossing edges
        per_tet = np.bincount(fto, minlength=c.T)                                         # 1: a one-triangle tet, 2: a two-triangle tet
        lo, hi = slice(0, tc.SECOND_PASS), slice(tc.SECOND_PASS, None)
        figures = {"crossing edges": (int(cross[lo].sum()), int(cross[hi].sum())),
                   "one-triangle tets": (int((per_tet[lo] == 1).sum()), int((per_tet[hi] == 1).sum())),
                   "two-triangle tets": (int((per_tet[lo] == 2).sum()), int((per_tet[hi] == 2).sum()))}
        print(f"two-pass: V {vo.shape[0]} F {fo.shape[0]}; below / from id 2^20: {figures}")
        assert all(a > 0 and b > 0 for a, b in figures.values())
        assert set(per_tet.tolist()) == {0, 1, 2}


@pytest.mark.parametrize("name", tc.SMALL_CASES)
def test_every_special_value_sits_on_a_crossing_edge(name):
    c = tc.case(name)
    edges = tc.case_tables(name)[0]
    key = {(int(a), int(b)): e for e, (a, b) in enumerate(edges)}
    fields, placements = tc.forward_fields(c), tc.special_placements(c)
    kinds = []
    for fname, placed in placements.items():
        sdf = fields[fname].numpy()
        cross = _crossing(c, sdf)
        for kind, a, b in placed:
            va, vb = tc.SPECIAL_KINDS[kind]
            assert cross[key[min(a, b), max(a, b)]], (fname, kind)
            assert np.float32(va).tobytes() == sdf[a].tobytes() and (isinstance(vb, int) or np.float32(vb).tobytes() == sdf[b].tobytes())
            kinds.append(kind)
        plain = np.ones(c.N, bool)
        plain[[v for _, a, b in placed for v in (a, b)]] = False
        assert np.array_equal(sdf[plain], tc.sdf_randn(c).numpy()[plain])                 # next to ordinary values
    assert sorted(kinds) == sorted(tc.SPECIAL_KINDS)
    z, placed = tc.zeros_field(c)
    z = z.numpy()
    assert sorted(k for k, _, _ in placed) == sorted(tc.ZERO_KINDS * (1 if name == "one-tet" else 4))
    assert int((z == 0).sum()) == len(placed) and int(np.signbit(z[z == 0]).sum()) == len(placed) // 2
    # torch.sign's mask counts edges that the > 0 test does not: the zero endpoint against a negative neighbour
    s = np.sign(z)
    by_sign = s[edges[:, 0]] != s[edges[:, 1]]
    assert (by_sign >= _crossing(c, z)).all() and (name == "one-tet" or int(by_sign.sum()) > int(_crossing(c, z).sum()))


# ---------------------------------------------------------------------------------------------------------------
# the oracle against the kernel's formulation
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.CASES)
def test_the_kernels_formulation_equals_the_oracle(name):
    c = tc.case(name)
    for fname, sdf in tc.forward_fields(c).items():
        vo, fo, fto = _oracle(c, sdf.numpy())
        v, f, ft, counts = tc.emulate_kernel(c.pos.numpy(), sdf.numpy(), c.tets, tables=tc.case_tables(name))
        assert tc.same_mesh((v, f, ft), (vo, fo, fto)), (name, fname)
        idx = tc.tet_sign_cases(sdf.numpy(), c.tets)
        assert counts == (vo.shape[0], fo.shape[0], int((tc.NUM_TRI[idx] == 1).sum()), int((tc.NUM_TRI[idx] == 2).sum()))
        assert not np.isnan(vo).any()                             # no finite pair with one endpoint > 0 makes 0 / 0 or inf / inf
        if fo.shape[0]:
            assert fo.min() == 0 and fo.max() == vo.shape[0] - 1
            uv = tc.uv_idx_of(fto, counts[2], c.T)
            assert uv.shape == fo.shape and uv[:, 0].max() == 4 * fto.max()
            assert set(tc.valid_vert_idx_of(fto, c.tets).tolist()) == set(c.tets[idx % 15 > 0].reshape(-1).tolist())


# (mutation, the cases that own the path, the fields on which they must catch it)
OWNERS = {"drop_carry": (("two-pass",), ("surface",)),
          "ge_zero": (tc.SMALL_CASES, ("special", "special:+0", "special:-0")),
          "two_tri_stride": (("T1023", "T1024", "T1025", "E1023", "E1024", "E1025", "N255", "N256", "N257", "star", "two-pass"),
                             ("randn", "surface")),
          "tet_chunk_base": (("T1025", "star", "two-pass"), ("randn", "surface"))}


@pytest.mark.parametrize("mut", tc.MUTATIONS)
def test_each_mutation_fails_on_the_case_that_owns_it(mut):
    owners, fields = OWNERS[mut]
    caught = {}
    for name in tc.CASES:
        if name == "two-pass" and name not in owners:
            continue                                              # a second of numpy per run: only where it is the owner
        c = tc.case(name)
        for fname, sdf in tc.forward_fields(c).items():
            got = tc.emulate_kernel(c.pos.numpy(), sdf.numpy(), c.tets, mut=mut, tables=tc.case_tables(name))
            caught[name, fname] = not tc.same_mesh(got, _oracle(c, sdf.numpy()))
    print(f"{mut}: caught by " + ", ".join(f"{n}/{f}" for (n, f), hit in caught.items() if hit))
    for name in owners:
        hits = [f for f in fields if caught.get((name, f))]
        assert hits, (mut, name)
        if mut == "ge_zero" and name == "one-tet":
            assert len(hits) == 2
    if mut == "drop_carry":                                       # and nothing below the edge can see them
        assert not any(hit for (n, f), hit in caught.items() if n != "two-pass")
    if mut == "tet_chunk_base":
        assert not any(hit for (n, f), hit in caught.items() if tc.case(n).T <= tc.CHUNK)


# ---------------------------------------------------------------------------------------------------------------
# host tables
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("star", "N257", "E1025", "one-tet"))
def test_build_incidence_against_a_loop(name):
    from meshdiffusion_amd.dmtet import build_incidence
    c = tc.case(name)
    edges = tc.case_tables(name)[0]
    ptr, inc = build_incidence(torch.from_numpy(edges).int(), c.N)
    want_ptr, want_inc = tc.incidence_brute_force(edges, c.N)
    assert ptr.dtype == torch.int32 and inc.dtype == torch.int32
    assert np.array_equal(ptr.numpy(), want_ptr) and np.array_equal(inc.numpy(), want_inc)
    inc = inc.numpy().astype(np.int64)
    assert np.array_equal(np.sort(inc), np.arange(2 * edges.shape[0]))                    # every edge twice, once per endpoint
    rows = np.diff(ptr.numpy())
    assert (rows[c.unnamed] == 0).all() and int((rows == 0).sum()) == c.unnamed.size
    for n in (0, c.N // 2, c.N - 1):
        row = inc[ptr[n]:ptr[n + 1]]
        assert (np.diff(row) > 0).all() and (edges[row >> 1, row & 1] == n).all()          # ascending, and they name the vertex
    if name == "star":
        assert rows[0] == tc.STAR_N + 2 and rows[-1] == 0
    with pytest.raises(ValueError):
        build_incidence(torch.from_numpy(edges).int(), int(edges.max()))                  # one vertex too few


@pytest.mark.parametrize("name", tc.SMALL_CASES)
def test_tet_tables_of_a_tet_list_in_an_unseen_order(name):
    """`TetTables` trusts the row order of torch.unique(dim=0, return_inverse=True): held against numpy's sorted keys on tets that
    are permuted, truncated and rotated."""
    from meshdiffusion_amd.dmtet import TetTables
    c = tc.case(name)
    tb = TetTables(torch.from_numpy(c.tets), "cpu")
    edges, tet_edges = tc.case_tables(name)
    assert (tb.n_tets, tb.n_edges) == (c.T, edges.shape[0])
    assert tb.edges.dtype == torch.int32 and np.array_equal(tb.edges.numpy(), edges)
    assert tb.tet_edges.dtype == torch.int32 and np.array_equal(tb.tet_edges.numpy(), tet_edges)
    assert np.array_equal(tb.tets.numpy(), c.tets) and torch.equal(tb.all_edges, torch.from_numpy(edges))
    import dmtet_grad_cases as dg
    assert torch.equal(dg.unique_edges(torch.from_numpy(c.tets)), torch.from_numpy(edges))


@pytest.mark.parametrize("kind", tc.GRID_MESHER_KINDS)
def test_grid_mesher_host_arithmetic_at_R7(kind):
    from meshdiffusion_amd.dmtet import GridMesher, grid_mask_from_tets, tet_vertices_to_grid_index
    v, t, grids = tc.grid_mesher_inputs(kind)
    idx = tet_vertices_to_grid_index(v)
    assert torch.equal(idx, torch.from_numpy(tc.kuhn(6, 6, 6)[0]).long())                 # the lattice coordinates, at any scale
    assert float(grid_mask_from_tets(v, 7).sum()) == 343
    mesher = GridMesher(v, t, 7, mesh_scale=2.1, deform_scale=2.0, device="cpu")
    pos, sdf = mesher.inputs(grids)
    assert int((grids[:, 1:].abs() > 1).sum()) > 100                                      # part of the deformation is clipped
    for m in range(grids.shape[0]):
        po, so = dmtet_oracle.grid_to_tet_inputs(grids[m].numpy(), v, mesh_scale=2.1, deform_scale=2.0, R=7)
        d = float(np.abs(pos[m].numpy() - po).max())
        print(f"{kind} mesh {m}: max |pos - oracle pos| {d:.3e}")
        assert np.array_equal(sdf[m].numpy(), so) and d <= 1e-6
        assert set(np.unique(so).tolist()) == {-1.0, 1.0}
