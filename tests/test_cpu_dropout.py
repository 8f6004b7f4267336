"""tests/dropout_cases.py, the host restatement of the training dropout mask (csrc/md_common.h), on its own: the threshold table,
pinned hash words, and the statistical properties a mask needs.  The statistics are a claim about the restatement only;
tests/test_gpu_dropout.py ties every kernel to it bit for bit."""
import numpy as np
import pytest

import dropout_cases as dc

# SplitMix64 of seed + (q + 1) * golden, computed once with Python integers (`% 2**64`), not with the numpy path under test.
# (0, 0) is the first output of the published SplitMix64 generator seeded with 0.
PINNED = (
    (0, 0, 0xE220A8397B1DCDAF),
    (0, 1, 0x6E789E6AA1B965F4),
    (1, 0, 0x910A2DEC89025CC1),
    (2 ** 64 - 1, 2 ** 32 + 5, 0x3235C18E80D1D10F),
)


@pytest.mark.parametrize("p,want", dc.THR16_TABLE)
def test_thr16_table(p, want):
    assert dc.thr16(p) == want
    if want == 0:
        assert dc.keep(5, p, 2, 16, 8, 8, 33).all()
        assert np.array_equal(dc.factor(5, p, 2, 16, 8, 8, 33), np.ones((2, 8, 33), np.float32))


def test_thr16_is_the_fp32_expression():
    """Values where fp32 and float64 disagree about p * 65536 + 0.5 do not exist below 2^24, but the ends do clamp."""
    assert dc.thr16(0.0) == 0 and dc.thr16(-1.0) == 0 and dc.thr16(1.0) == 65535 and dc.thr16(0.9999999) == 65535
    assert dc.thr16(2.0 ** -17 * 0.999) == 0 and dc.thr16(1.5 / 65536) == 2 and dc.thr16(1.49 / 65536) == 1
    assert dc.scale(0.5) == np.float32(2) and dc.scale(0.1).dtype == np.float32
    assert float(dc.scale(0.1)) == float(np.float32(1) / np.float32(0.9))


def test_hash_words_pinned():
    for seed, q, want in PINNED:
        assert dc.hash_word_int(seed, q) == want
        assert int(dc.hash_words(seed, np.array([q], dtype=np.uint64))[0]) == want
    # step by step for (0, 0): z0 = golden; each line is one statement of md_drop_bits
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert z ^ (z >> 31) == PINNED[0][2]


def test_fields_and_quad_index_by_hand():
    """Element (b, channel, pos) reads field (b * c_total + channel) & 3 of the word of quad ((b * c_total + channel) >> 2) * P + pos;
    field 0 is the low 16 bits; c_off moves the channel, not the word."""
    B, c_total, c_off, C, P, seed = 2, 24, 8, 16, 5, 99
    f = dc.fields(seed, B, c_total, c_off, C, P)
    for b, c, pos in ((0, 0, 0), (0, 3, 4), (1, 5, 2), (1, 15, 4)):
        n = b * c_total + c_off + c
        w = dc.hash_word_int(seed, (n // 4) * P + pos)
        assert int(f[b, c, pos]) == (w >> (16 * (n % 4))) & 0xFFFF
    whole = dc.fields(seed, B, c_total, 0, c_total, P)
    assert np.array_equal(whole[:, c_off:c_off + C], f)
    k = dc.keep(seed, 0.5, B, c_total, c_off, C, P)
    assert np.array_equal(k, f >= 32768)
    fac = dc.factor(seed, 0.5, B, c_total, c_off, C, P)
    assert fac.dtype == np.float32 and set(np.unique(fac).tolist()) == {0.0, 2.0} and np.array_equal(fac != 0, k)


@pytest.mark.parametrize("p", dc.STAT_PS)
@pytest.mark.parametrize("seed", dc.STAT_SEEDS)
def test_mask_statistics(seed, p):
    """Marginal keep rate and the phi coefficient x sqrt(n) of five kinds of neighbours: every |z| <= 5 (measured: worst 2.39 over
    the 180 statistics).  Per-field keep rate (channel-in-quad 0..3) within 5 sigma."""
    t16 = dc.thr16(p)
    k, pairs = dc.stat_pairs(seed, p)
    assert k.shape == (4, 32, 4096)
    zs = {"keep rate": dc.rate_z(k, t16)}
    zs.update({name: dc.phi_z(a, b) for name, (a, b) in pairs.items()})
    for e in range(4):
        zs[f"field {e} keep rate"] = dc.rate_z(k[:, e::4], t16)
    print(f"seed {seed:#x} p {p}: " + ", ".join(f"{n} {z:+.2f}" for n, z in zs.items()))
    for name, z in zs.items():
        assert abs(z) <= dc.STAT_Z, (name, z)


def test_phi_z_sees_a_shared_word():
    """The statistic has teeth: a mask whose odd channels repeat the even ones' field, or whose seeds are 1 apart in q, is far out."""
    k = dc.keep(3, 0.3, **dc.STAT_SHAPE)
    assert abs(dc.phi_z(k[:, 0::2], k[:, 0::2])) > 100
    f = dc.fields(3, **dc.STAT_SHAPE)
    low_byte_twice = (f & 0xFF) >= 77                  # two fields cut from overlapping bits of one word
    overlapped = ((f >> 4) & 0xFF) >= 77
    assert abs(dc.phi_z(low_byte_twice, overlapped)) > 5
