"""Host-side checks of meshdiffusion_amd/fit.py that need no GPU: the Huber step and the three depth terms that parameterise it
against values worked out by hand, the vertex-to-pixel helper of both carves, the re-exports, and the loop driver on a stub."""
import types

import pytest
import torch

from meshdiffusion_amd import fit


def test_huber_step_values_and_gradients():
    d = torch.tensor([0.5, 1.0, 2.0], requires_grad=True)
    out = fit._huber(d)
    out.sum().backward()
    assert out.tolist() == [0.5, 1.0, 4.0]                                  # d below 1, d^2 from 1 on
    assert d.grad.tolist() == [1.0, 2.0, 4.0]


def _hand_target():
    """One view of 2 x 2 pixels.  Pixel (0,0): covered, two layers 0.5 apart.  (0,1): covered, layers closer than 5e-3.
    (1,0): mask 0.5 (an antialiased edge).  (1,1): no second layer (-1)."""
    px = lambda *v: torch.tensor(v, dtype=torch.float32).reshape(1, 2, 2, 1)     # noqa: E731
    target = {"depth": px(2.0, 2.0, 2.0, 2.0), "depth_second": px(2.5, 2.001, 2.5, -1.0), "mask_cont": px(1.0, 1.0, 0.5, 1.0)}
    buffers = {"depth": px(2.25, 5.0, 4.0, 3.0), "depth_second": px(3.0, 2.5, 42.5, 0.0)}
    return buffers, target


def test_depth_terms_on_a_hand_made_target():
    buffers, target = _hand_target()
    # tick: d1 = |0.25|, |3| at the two exact-mask, valid pixels -> 0.25 + 9; d2 = 0.5 * 0.1 at the one pixel that is also apart
    assert float(fit.depth_loss(buffers, target, 0)) == pytest.approx(((0.25 + 9.0) / 4 + 0.05 / 4) * 100.0, rel=1e-6)
    assert float(fit.depth_loss(buffers, target, 10000)) == pytest.approx((0.25 + 9.0) / 4 + 0.05 / 4, rel=1e-6)
    # fixed topology: second layer only, the mask as it is: 0.5 * 0.1 at (0,0), 40 * 0.5 * 0.1 = 2 -> 4 at (1,0)
    assert float(fit.depth_loss_fixedtopo(buffers, target)) == pytest.approx((0.05 + 4.0) / 4 * 100.0, rel=1e-6)
    # single view: layer 1 only, exact mask, both gates: only (0,0) survives
    assert float(fit.depth_loss_single_view(buffers, target)) == pytest.approx(0.25 / 4 * 100.0, rel=1e-6)
    moved = {**buffers, "depth": buffers["depth"] + 1.0}
    assert float(fit.depth_loss_fixedtopo(moved, target)) == float(fit.depth_loss_fixedtopo(buffers, target))   # layer 1 does not enter


def test_vertex_pixels_round_or_truncate():
    # an identity camera: unit coordinates 0.5 x + 0.5 -> 0.6 and 0.4, times (W - 1, H - 1) = (4, 2) -> 2.4 and 0.8; outside -> clipped
    geo = types.SimpleNamespace(get_deformed=lambda: torch.tensor([[0.2, -0.2, 0.0], [3.0, -3.0, 0.0]]))
    target = {"resolution": [3, 5], "mvp": torch.eye(4)[None]}
    px, py = fit._vertex_pixels(geo, target, rounded=True)
    assert px.tolist() == [[2, 4]] and py.tolist() == [[1, 0]] and px.dtype == torch.int64
    px, py = fit._vertex_pixels(geo, target, rounded=False)
    assert px.tolist() == [[2, 4]] and py.tolist() == [[0, 0]]


def test_old_modules_hand_out_the_moved_names():
    from meshdiffusion_amd import pointcloud, render, singleview
    for module in (render, pointcloud, singleview):
        for name in module._IN_FIT:
            assert getattr(module, name) is getattr(fit, name), name
        with pytest.raises(AttributeError):
            module.no_such_name


@pytest.mark.parametrize("iters, start", ((3, 0), (2, 7), (0, 5)))
def test_driver_on_a_stub(iters, start):
    x = torch.nn.Parameter(torch.tensor(4.0))
    clamps, calls = [], []
    geo = types.SimpleNamespace(clamp_deform=lambda: clamps.append(float(x.detach())))
    opt = torch.optim.SGD([x], lr=0.5)

    def step(it):
        assert x.grad is None                                                # zero_grad came first
        return x * 2.0, {"twice": x * 2.0, "it": torch.tensor(float(it)), "unused": None}, f"mesh {it}"
    out = fit._optimise(geo, opt, iters, step, ("twice", "it"), lambda it, term, mesh: calls.append((it, float(term), mesh)),
                        torch.device("cpu"), start)
    assert sorted(out) == ["it", "twice"] and all(t.shape == (iters,) and not t.requires_grad for t in out.values())
    assert out["it"].tolist() == [float(start + k) for k in range(iters)]
    assert out["twice"].tolist() == [8.0 - 2.0 * k for k in range(iters)]    # x falls by lr * 2 per step; the term is from before it
    assert clamps == [4.0 - (k + 1) for k in range(iters)]                   # clamp_deform after the step
    assert calls == [(start + k, 8.0 - 2.0 * k, f"mesh {start + k}") for k in range(iters)]   # the headline term is names[0]


def test_driver_steps_the_scheduler_after_the_optimiser():
    x = torch.nn.Parameter(torch.tensor(1.0))
    opt = torch.optim.SGD([x], lr=1.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda it: 0.5 ** it)
    geo = types.SimpleNamespace(clamp_deform=lambda: None)
    fit._optimise(geo, opt, 3, lambda it: (x * 1.0, {"x": x}, None), ("x",), None, torch.device("cpu"), sched=sched)
    assert float(x.detach()) == 1.0 - (1.0 + 0.5 + 0.25)
