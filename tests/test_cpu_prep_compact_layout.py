"""Host replay (no GPU) of the Winograd conv's halo addressing on the COMPACT upsampled operand (csrc/conv3_wino.hip, halo_off with
WnArgs::ups_dh; operand from md_wino_prep_upsdh) against the full layout of md_wino_prep(ups = 1).

The full operand holds row (z, y) of every (channel group, frequency, plane) slice; after nearest-x2 upsampling rows (2z' + i, 2y' + j)
are the same bits, and the compact operand holds row (z', y') once.  For every tile of an 8 x 16 x 16 output grid and every entry of
the 15 halo pieces: the same entries are live, a live entry's compact offset stays inside the compact chunk and names the item the
full offset names."""
import numpy as np

TZ, TY, TX = 4, 8, 8              # WN_TZ, WN_TY, WN_TX: output tile of a workgroup
TPOS, NDMA = 6 * 10 * 4, 15       # WN_TPOS: (dz, hy, pair) entries per (channel group half, plane); WN_NDMA pieces of 64 entries


def _halo_off(k, lane, z0, y0, x0, D, H, W, ups_dh):
    """halo_off of csrc/conv3_wino.hip: offset in 16-byte items relative to the (sample, chunk, frequency) base, -1 = outside the grid."""
    Wp = W >> 1
    Ph = (D * H * W) >> (1 + 2 * ups_dh)
    e = k * 64 + lane
    hp, tp = divmod(e, TPOS)
    dz, hy, pr = tp // 40, (tp >> 2) % 10, tp & 3
    z, y = z0 + dz - 1, y0 + hy - 1
    live = 0 <= z < D and 0 <= y < H
    row = (z >> ups_dh) * (H >> ups_dh) + (y >> ups_dh)
    off = (hp >> 1) * 8 * Ph + (hp & 1) * Ph + row * Wp + (x0 >> 1) + pr
    return off if live else -1


def test_compact_halo_offsets_name_the_items_of_the_full_layout():
    D, H, W = 8, 16, 16
    Wp, Ph, Phc = W // 2, D * H * W // 2, D * H * W // 8
    rng = np.random.default_rng(5)
    # one chunk (two channel groups) of one frequency: [cg 2][f 4][plane 2][rows][Wp]; the kernel's base selects f, so f = 0 here
    src = rng.integers(1, 1 << 60, size=(2, 4, 2, D // 2, H // 2, Wp), dtype=np.int64)       # the compact operand: one value per item
    full = np.repeat(np.repeat(src, 2, axis=3), 2, axis=4)                                    # rows (2z' + i, 2y' + j) duplicate it
    assert full.shape == (2, 4, 2, D, H, Wp)
    cflat, fflat = src.reshape(-1), full.reshape(-1)
    assert cflat.size == 16 * Phc and fflat.size == 16 * Ph
    seen_rows = set()
    n_live = n_dead = 0
    for z0 in range(0, D, TZ):
        for y0 in range(0, H, TY):
            for x0 in range(0, W, TX):
                for k in range(NDMA):
                    for lane in range(64):
                        of = _halo_off(k, lane, z0, y0, x0, D, H, W, 0)
                        oc = _halo_off(k, lane, z0, y0, x0, D, H, W, 1)
                        assert (of < 0) == (oc < 0), (z0, y0, x0, k, lane)          # liveness is the full-resolution row's
                        if of < 0:
                            n_dead += 1
                            continue
                        n_live += 1
                        assert 0 <= oc < 16 * Phc and 0 <= of < 16 * Ph
                        assert cflat[oc] == fflat[of], (z0, y0, x0, k, lane)
                        seen_rows.add((oc % Phc) // Wp)
    assert n_dead > 0 and n_live > 0                       # both halo faces of the grid were met
    assert seen_rows == set(range((D // 2) * (H // 2)))   # every compact row is read, interior duplicates included

