"""Host replay (no GPU) of md_block_pass_kernel's lane map (csrc/block_pass.hip) for W = 32 and W = 64.

A wave owns 32 consecutive positions of a 256-position tile; lane (j, h) holds channel group h of the K block at position j.
Replayed here, for every wave and lane of a tile:
  the neighbour choice -- lane - 1 / lane + 1, the halo holder lane 8 k + 4 h + 2 end + half at the ends of the segment, zero at
  the ends of a row -- must name position x - 1 / x + 1 of the SAME row and the same channels, and a holder loads only inside the row;
  the frequency pair a lane forms (even position of a pair: f0, f1 from d0 d1 d2; odd: f2, f3 from d1 d2 d3) and the swap of the
  upper 32 lanes of the first with the lower 32 lanes of the second: every lane ends with ONE frequency 2 (j & 1) + h of pair
  j >> 1, channel group 0 in the first half and 1 in the second;
  the four stores per lane and K block: every 16-byte item of the tile's part of T[B][C/8][4][2][P/2] is written exactly once, and
  it is the item md_wino_prep2_f6_kernel's (pair, frequency half) map writes for that (pair, frequency, channel group, plane)."""
import numpy as np
import pytest

TILE, WAVES, GS = 256, 8, 4


def _neighbour(W, wid, j, h, k, side):
    """What lane (j, h) of wave `wid` takes as its left (side = -1) / right (+1) neighbour at step k of a group: ("zero",) |
    ("lane", lane) | ("halo", holder lanes of the two 16-byte halves)."""
    xr = (wid * 32 + j) & (W - 1)
    if (side < 0 and xr == 0) or (side > 0 and xr == W - 1):
        return ("zero",)
    if (side < 0 and j == 0) or (side > 0 and j == 31):
        end = 1 if j == 31 else 0
        return ("halo", [8 * k + 4 * h + 2 * end + half for half in (0, 1)])
    return ("lane", ((h * 32 + j) + side) & 63)


def _holder(W, wid, L):
    """Halo holder lane L < 32 -> (step, channel group, position relative to the tile, half) or None where it does not load."""
    hk, hh, hend, hq = (L >> 3) & 3, (L >> 2) & 1, (L >> 1) & 1, L & 1
    seg_l, seg_r = ((wid * 32) & (W - 1)) != 0, ((wid * 32 + 32) & (W - 1)) != 0
    if not (seg_r if hend else seg_l):
        return None
    return hk, hh, wid * 32 + (32 if hend else -1), hq


@pytest.mark.parametrize("W", [32, 64])
def test_neighbours_and_halo_name_the_adjacent_position_of_the_same_row(W):
    n_halo = n_zero = 0
    for wid in range(WAVES):
        for L in range(32):
            hd = _holder(W, wid, L)
            if hd is not None:                      # a holder loads inside the tile, and inside the row of the segment's end
                pos = hd[2]
                assert 0 <= pos < TILE
                edge = wid * 32 + (31 if pos > wid * 32 else 0)
                assert pos // W == edge // W
        for k in range(GS):
            for h in range(2):
                for j in range(32):
                    pos = wid * 32 + j
                    for side in (-1, 1):
                        src = _neighbour(W, wid, j, h, k, side)
                        inside = 0 <= pos % W + side < W
                        if src[0] == "zero":
                            n_zero += 1
                            assert not inside
                        elif src[0] == "lane":
                            assert inside and src[1] >> 5 == h and wid * 32 + (src[1] & 31) == pos + side
                        else:
                            n_halo += 1
                            for half, L in enumerate(src[1]):
                                assert L < 32 and _holder(W, wid, L) == (k, h, pos + side, half)
                            assert inside
    # W = 32: a segment is a row, both ends are padding; W = 64: the interior end of every segment comes from the halo
    assert n_halo == (0 if W == 32 else WAVES * GS * 2) and n_zero == WAVES * GS * 2 * (2 if W == 32 else 1)


def test_swap_leaves_one_frequency_and_both_channel_groups_per_lane():
    fa = [(2 * (j & 1) + 0, j >> 1, h) for h in range(2) for j in range(32)]      # lane -> (frequency, pair, channel group)
    fb = [(2 * (j & 1) + 1, j >> 1, h) for h in range(2) for j in range(32)]
    a, b = list(fa), list(fb)
    a[32:], b[:32] = fb[:32], fa[32:]               # v_permlane32_swap: the first operand's upper row <-> the second's lower row
    seen = set()
    for lane in range(64):
        j, h = lane & 31, lane >> 5
        assert a[lane] == (2 * (j & 1) + h, j >> 1, 0) and b[lane] == (2 * (j & 1) + h, j >> 1, 1)
        seen.add(a[lane][:2])
    assert len(seen) == 64                          # 16 pairs x 4 frequencies


@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("K", [128, 256])
def test_every_item_of_a_tile_is_written_exactly_once(W, K):
    Bn, D, H = 2, 2, 512 // W                       # P = 1024: 4 tiles per sample
    P = D * H * W
    Ph, CG = P // 2, K // 8
    count = np.zeros(Bn * CG * 8 * Ph, dtype=np.int32)
    what = np.full((Bn * CG * 8 * Ph, 5), -1, dtype=np.int64)      # (sample, pair, frequency, channel group, plane) written there
    for b in range(Bn):
        for tile in range(P // TILE):
            p0 = tile * TILE
            for ks in range(K // 16):
                for wid in range(WAVES):
                    tb = ((b * CG + 2 * ks) * 8) * Ph + ((p0 + wid * 32) >> 1)
                    for lane in range(64):
                        j, h = lane & 31, lane >> 5
                        f = 2 * (j & 1) + h
                        voff = 2 * f * Ph + (j >> 1)
                        for g2, plane in ((0, 0), (0, 1), (1, 0), (1, 1)):      # h0, q0, h1, q1
                            o = tb + voff + g2 * 8 * Ph + plane * Ph
                            count[o] += 1
                            what[o] = (b, (p0 + wid * 32) // 2 + (j >> 1), f, 2 * ks + g2, plane)
    assert count.min() == 1 and count.max() == 1
    # md_wino_prep2_f6_kernel: out0 = T + ((b CG + 2 cgp) 8) Ph + pos2, item (f 2 + plane) Ph, the second group 8 Ph further
    idx = np.arange(Bn * CG * 8 * Ph)
    pos2, plane, f, cg, b = idx % Ph, (idx // Ph) % 2, (idx // (2 * Ph)) % 4, (idx // (8 * Ph)) % CG, idx // (8 * Ph * CG)
    assert np.array_equal(what, np.stack([b, pos2, f, cg, plane], axis=1))
