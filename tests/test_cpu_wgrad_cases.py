"""What the bit-for-bit weight-gradient tests (tests/test_gpu_wgrad_exact.py) rest on, proven without a GPU: for every case of
tests/wgrad_cases.py, in the domain of the kernel it is fed to (the tensors themselves for md_wgrad / md_wgrad_nin, T = B^T d
and U = (dy0, dy0 + dy1, dy0 - dy1, dy1) for md_wgrad_wino), (a) the hi / lo split reproduces every operand and no lo * lo pair
is non-zero, (b) the lo plane the class names is live THERE and the other one is zero, (c) sum |term| stays below 2^24 for
every accumulator, the non-zero integer dW0 included -- per tap, or per frequency, for the reduce kernel's 0.5f (n1 +- n2) and
for the three taps it writes, (d) an fp32 evaluation of the three terms in two summation orders with two different K splits
equals the float64 reference bit for bit, and (e) the reference itself equals float64 autograd of nn.Conv3d (stride 2 and
nearest x2 included) and the restated PB16 z-slab layout + slot -> tap map of md_wgrad.  With that a mismatch on the GPU is
the kernel's.  The host-side refusals of the three entry points that no other test pins are at the end."""
import pytest
import torch

import wgrad_cases as wc


@pytest.mark.parametrize("case_id", wc.IDS)
def test_case_is_exact_in_the_domain_it_is_fed_to(case_id):
    spec = wc.spec_of(case_id)
    case = wc.build(spec)
    domain = wc.domain_of(spec)
    for t in (case["a"], case["dy"], case["dw0"]):
        assert t.dtype == torch.float32 and torch.equal(t, t.round())
    assert bool((case["dw0"] != 0).all()), "dW0 has to be non-zero everywhere"
    m = wc.exactness_margin(case, domain)
    assert m["split_exact"], f"{case_id} [{domain}]: hi + lo does not reproduce an operand"
    assert m["lolo_zero"], f"{case_id} [{domain}]: a lo * lo product is non-zero"
    assert m["dy_even"], f"{case_id} [{domain}]: an odd dY-side operand (0.5f (n1 +- n2) would leave the integers)"
    worst = max(m["max_sum"].items(), key=lambda kv: kv[1])
    print(f"{case_id} [{domain}]: max sum |term| = 2^24 x {worst[1] / wc.LIMIT:.3f} ({worst[0]})")
    for name, v in m["max_sum"].items():
        assert v < wc.LIMIT, f"{case_id} [{domain}]: sum |term| of {name} = {v:.4g} >= 2^24"
    live = dict(hi_only=(False, False), a_lo=(True, False), dy_lo=(False, True))[spec["cls"]]
    assert all(v == live[0] for v in m["a_lo_live"]) and all(v == live[1] for v in m["dy_lo_live"]), \
        f"{case_id} [{domain}]: lo planes A {m['a_lo_live']} dY {m['dy_lo_live']}"
    ref = wc.reference(case)
    assert bool((ref != case["dw0"].double()).any()) and torch.equal(ref, ref.round())
    for order in (0, 1):
        got = wc.eval_fp32(case, domain, order)
        msg = wc.describe_mismatch(got.double(), ref, f"{case_id} [{domain}] fp32 evaluation, order {order}")
        assert not msg, msg
    # the reference against float64 autograd on rows and columns spread over the tiles
    rows = sorted({0, 1, case["co"] // 2, case["co"] - 1})
    cols = sorted({0, case["ci"] // 3, case["ci"] - 2, case["ci"] - 1})
    assert torch.equal(ref[rows][:, cols], wc.autograd_reference(case, rows, cols)), f"{case_id}: the tap-wise reference is not the autograd gradient"
    # every element of dW has its own float; the surplus channels of the operand tensors are live
    idx = wc.dw_index(case)
    assert idx.unique().numel() == idx.numel() and int(idx.min()) == 0
    if case["a_ch"] > case["co"]:
        assert bool(case["dy"][:, case["co"]:].any())
    if case["b_ch"] > case["ci"]:
        assert bool(case["a"][:, case["ci"]:].any())
    if spec["entry"] == "pb":
        msg = wc.describe_mismatch(wc.pb16_model(case), ref, f"{case_id}: md_to_pb16 + md_wgrad restated (z-slabs, slot -> tap map)")
        assert not msg, msg


def test_classes_differ_where_they_claim():
    """A dropped cross term is visible: the reference changes when the live lo plane is removed, in every entry's domain."""
    for entry in ("pb", "wino", "nin"):
        for cls, side in (("a_lo", "a"), ("dy_lo", "dy")):
            case = wc.build(next(s for s in wc.SPECS if s["cls"] == cls and s["entry"] == entry))
            broken = dict(case)
            broken[side] = wc.split_bf16(case[side])[0]
            assert not torch.equal(wc.reference(broken), wc.reference(case)), (entry, cls)


def test_zslab_layout_is_what_makes_the_slab_sum_the_whole_sum():
    """The restated layout itself: with the activation's z-halo planes zeroed (zhalo = 0 on A) or the dY halo planes filled with
    the neighbour's (zhalo = 1 on dY), the slab-wise contraction is NOT the gradient -- the model tells the two apart."""
    spec = wc.spec_of("pb-27-hi_only-4x4x4-128x128-B3-zslab")
    case = wc.build(spec)
    zs = wc.zsplit_for(case["B"], 4)
    assert zs == 4 and [wc.zsplit_for(b, 8) for b in (1, 3, 6, 8, 11)] == [8, 8, 4, 1, 8] and wc.zsplit_for(2, 16) == 4
    a = wc.act_full(case)[:, :8]
    with_halo, without = wc.pb16_values(a, zs, 1, 1, 4), wc.pb16_values(a, zs, 1, 0, 4)
    assert with_halo.shape == (16, 8, 4 + 3 * 36 + 4) and not torch.equal(with_halo, without)
    assert not bool(with_halo[12:].any()) and not bool(with_halo[:, :, :4].any()) and not bool(with_halo[:, :, -4:].any())
    # slab 1 of sample 0: its lower halo plane is plane 0 of the sample, its interior plane 1, its upper halo plane 2
    blk = with_halo[1, :, 4:-4].reshape(8, 3, 6, 6)
    assert torch.equal(blk[:, :, 1:5, 1:5], a[0, :, 0:3]) and not bool(without[1, :, 4:-4].reshape(8, 3, 6, 6)[:, (0, 2)].any())


def test_slot_tap_map_of_the_5x5x5_form():
    """150 slots = 50 groups x 3; 125 of them are the taps, each once, and the 25 discarded ones are exactly dx = +3."""
    st = wc.slot_taps(125)
    assert [s for s, _, _ in st] == list(range(150))
    assert sorted(t for _, t, _ in st if t is not None) == list(range(125))
    assert all(off[2] == 3 for _, t, off in st if t is None) and sum(t is None for _, t, _ in st) == 25
    for _, t, (dz, dy, dx) in st:
        if t is not None:
            assert t == ((dz + 2) * 5 + dy + 2) * 5 + dx + 2
    assert [t for _, t, _ in wc.slot_taps(27)] == list(range(27)) and wc.slot_taps(27)[0][2] == (-1, -1, -1)


def test_case_table_reaches_the_paths_it_names():
    """The table itself, against the launch arithmetic of csrc/wgrad.hip / wgrad_wino.hip restated here."""
    pb = [s for s in wc.SPECS if s["entry"] == "pb"]

    def stages(s):
        D, H, _ = s["dims"]
        zs = wc.zsplit_for(s["B"], D)
        return (s["B"] * zs + 7) // 8 * (D // zs) * H * ((H + 7) // 8)

    def units(s):
        return ((s["co"] + 127) // 128) * ((s["ci"] + 127) // 128) * {27: 9, 125: 50, 1: 1}[s["taps"]]

    full = lambda s: s["co"] % 128 == 0 and s["ci"] % 128 == 0 and s["dims"][1] % 8 == 0
    for taps in (27, 1):
        assert any(full(s) for s in pb if s["taps"] == taps) and any(not full(s) for s in pb if s["taps"] == taps)
    assert {s["dims"][1] % 8 for s in pb if s["taps"] == 27} == {0, 4}
    for cls in wc.CLASSES:
        for entry in ("pb", "wino", "nin"):
            assert any(s["cls"] == cls and s["entry"] == entry for s in wc.SPECS), (cls, entry)
        assert any(s["cls"] == cls and s["taps"] == 125 for s in pb) and any(s["cls"] == cls and s["taps"] == 1 for s in pb)
    ks = lambda s: [k for k in s["ksplit"] if k is not None]
    assert any(k * units(s) > 256 for s in pb for k in ks(s)), "no case reaches the second round of the XCD remap"
    assert any(stages(s) % k for s in pb for k in ks(s)), "no K split that does not divide the stages"
    assert any((stages(s) + k - 1) // k * (k - 1) >= stages(s) for s in pb for k in ks(s) if k > 1), "no empty K range"
    assert {wc.zsplit_for(s["B"], s["dims"][0]) for s in pb} == {1, 2, 4, 8}
    assert any(s["dims"][0] // wc.zsplit_for(s["B"], s["dims"][0]) == 1 and (s["B"] * wc.zsplit_for(s["B"], s["dims"][0])) % 8 for s in pb)
    assert any(s["dims"][0] != s["dims"][1] for s in pb)
    # the reduce kernels: md_wgrad_reduce27_kernel needs s_k == 27, s_tap == 1, cols % 64 == 0
    r27 = lambda s: s["taps"] == 27 and wc.strides_of(s)[1:] == (27, 1) and s["ci"] % 64 == 0
    assert any(r27(s) for s in pb) and any(s["taps"] == 27 and not r27(s) and s["ci"] % 64 == 0 for s in pb) \
        and any(s["taps"] == 27 and s["ci"] % 64 for s in pb)
    wino = [s for s in wc.SPECS if s["entry"] == "wino"]
    assert {s["dims"][2] for s in wino} == {32, 64} and {s["B"] for s in wino} == {1, 2, 3}
    assert {(s["co"], s["ci"]) for s in wino} == {(128, 128), (256, 128), (128, 256)}
    for s in wino:
        D, H, W = s["dims"]
        assert 256 % W == 0 and (D * H * W) % 256 == 0 and D >= 2 and H >= 2              # the operand passes' and the kernel's contracts
        assert all(1 <= k <= s["B"] * (D - 1) for k in ks(s))
    assert any(s["B"] * (s["dims"][0] - 1) in ks(s) for s in wino) and any((s["B"] * s["dims"][0]) % k for s in wino for k in ks(s))
    # streams that are no multiple of the 4-step unroll, and one of a single plane and a few rows
    steps = lambda s, planes: planes * (s["dims"][1] + 1) * (s["dims"][2] // 32) + s["dims"][2] // 32
    assert any(steps(s, 1) % 4 for s in wino if s["B"] * (s["dims"][0] - 1) in ks(s)) and min(steps(s, 1) for s in wino) <= 4
    nin = [s for s in wc.SPECS if s["entry"] == "nin"]
    assert {s["dims"][2] for s in nin} == {16, 48, 4096} and {s["B"] for s in nin} == {1, 3}
    for s in nin:
        ne = s["B"] * s["dims"][2] // 16
        assert all(1 <= k <= ne for k in ks(s))
    assert any(s["B"] * s["dims"][2] // 16 in ks(s) for s in nin)
    # a range boundary strictly inside a sample: e = NE r / ksplit not a multiple of the elements per sample
    assert any((s["B"] * s["dims"][2] // 16 * r // k) % (s["dims"][2] // 16) for s in nin if s["B"] > 1 for k in ks(s) for r in range(1, k))


@pytest.mark.parametrize("B,c,dims", wc.DUAL_CASES)
def test_dual_pass_inputs_are_exact(B, c, dims):
    """md_wino_prep_dual's own cases: T and U are integers of at most 12 bits (hi + lo exact, lo planes live) and every channel sum
    is exact in fp32 whatever the order."""
    x = wc.dual_input(B, c, dims)
    assert 256 % dims[2] == 0 and (dims[0] * dims[1] * dims[2]) % 256 == 0
    for t in wc.wino_T(x) + wc.wino_U(x):
        hi, lo = wc.split_bf16(t)
        assert torch.equal(hi + lo, t) and bool(lo.any())
    assert float(x.abs().sum(dim=(2, 3, 4)).max()) < wc.LIMIT


def test_host_side_refusals(hip_lib):
    """Shapes the headers exclude, refused before any launch (dummy pointers are never dereferenced)."""
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p, big = ctypes.cast(buf, ctypes.c_void_p), 1 << 40
    g8 = 1 * (10 * 10 + 10 + 1) + 10                                                               # S = 8, pad 1: the smallest guard
    assert hip_lib.md_wgrad(p, p, p, p, big, 8, 128, 128, 128, 128, 8, 8, 4, g8, 27, 1, 27 * 128, 27, 1, None) == -1     # W != H
    assert hip_lib.md_wgrad(p, p, p, p, big, 8, 128, 128, 128, 128, 8, 4, 8, g8, 27, 1, 27 * 128, 27, 1, None) == -1
    assert hip_lib.md_wgrad(p, p, p, p, big, 8, 128, 128, 128, 128, 8, 8, 8, g8 - 1, 27, 1, 27 * 128, 27, 1, None) == -1  # guard one short
    g5 = 2 * (12 * 12 + 12 + 1) + 10
    assert hip_lib.md_wgrad(p, p, p, p, big, 8, 128, 8, 128, 4, 8, 8, 8, g5 - 1, 125, 1, 4 * 125, 125, 1, None) == -1     # pad 2 needs twice the rows
    assert hip_lib.md_wgrad(p, p, p, p, big, 8, 128, 8, 128, 4, 8, 8, 8, g8, 125, 1, 4 * 125, 125, 1, None) == -1
    assert hip_lib.md_wgrad(p, p, p, p, big, 8, 128, 128, 136, 128, 8, 8, 8, g8, 27, 1, 27 * 128, 27, 1, None) == -1      # rows > a_ch
    assert hip_lib.md_wgrad(p, p, p, p, big, 8, 128, 128, 128, 128, 8, 8, 8, g8, 9, 1, 27 * 128, 27, 1, None) == -1       # taps
    assert hip_lib.md_wgrad_nin(p, p, p, p, big, 1, 128, 128, 24, 1, 1, 128, None) == -2                                  # P % 16
    assert hip_lib.md_wgrad_nin(p, p, p, p, big, 1, 128, 128, 8, 1, 1, 128, None) == -2
    assert hip_lib.md_wgrad_nin(p, p, p, p, big, 3, 128, 128, 48, 10, 1, 128, None) == -1                                 # ksplit > B P / 16
    assert hip_lib.md_wgrad_nin(p, p, p, p, big, 1, 128, 96, 48, 1, 1, 128, None) == -2
    # the operand passes of md_wgrad_wino: whole rows per workgroup, so (2, 2, 32) is below the smallest grid and (2, 4, 32) is not
    assert hip_lib.md_wino_prep_dual(p, None, 8, 0, None, 0, 0, p, p, None, 1, 2, 2, 32, 0.0, 0, None) == -2
    assert hip_lib.md_wino_prep_v2(p, None, 8, 0, None, 0, 0, p, 1, 2, 6, 32, 0.0, 0, None) == -2
    assert hip_lib.md_wino_prep_dual(p, None, 8, 0, None, 0, 0, p, p, None, 1, 4, 4, 24, 0.0, 0, None) == -2              # W does not divide 256
    assert hip_lib.md_wgrad_wino(p, p, p, p, big, 1, 128, 128, 1, 8, 32, 1, 27 * 128, 27, 1, None) == -2                  # D < 2
    assert hip_lib.md_wgrad_wino(p, p, p, p, big, 1, 128, 128, 8, 1, 32, 1, 27 * 128, 27, 1, None) == -2
    assert hip_lib.md_wgrad_wino(p, p, p, p, big, 2, 128, 128, 4, 2, 32, 7, 27 * 128, 27, 1, None) == -1                  # ksplit > B (D - 1) = 6
