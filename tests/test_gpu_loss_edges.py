"""GPU: csrc/gnode_loss.hip (k_l1_loss, k_l1_reduce) at the shapes its launcher treats differently.

The launcher takes  RB = clamp(max(4, ceil(rows / kLossGrid)), 1, min(64, 48 KB / per_row))  rows per workgroup
(per_row = 3 T sizeof(label)) and at most kLossGrid = 1024 workgroups; past that the workgroups walk the row blocks in
a grid-stride loop and restage their LDS.  test_gpu_trainer.py's cases stay below 4 097 rows and T = 200: no wrap, no
LDS cap.  Here: the wrap (more than 65 536 rows), the 48 KB cap down to RB = 1 at exactly 48 KB of dynamic LDS next to
the 2 KB static reduction buffer, one element, t0 = T, the first T that does not fit, and the sign_scale path of
l1_loss_mean_backward.

Reference and bars are test_fused_l1_loss_matches_the_torch_expression's: the torch expression the reference evaluates
(ode_nn_ngraph_sim.py:230-234) with autograd's gradient; value within 1e-12 relative (float64 summation order),
gradient torch.equal, a second run bitwise equal; exact ties on every third row.  `_regime` restates the launcher's
arithmetic so that every case asserts the RB and block count it is here for.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOSS_GRID = 1024                      # kLossGrid of csrc/gnode_loss.hip
LDS_CAP = 48 * 1024


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gnode import _lib
    _lib.load()                       # fails loudly if libgnode_hip.so is missing
    return torch.device("cuda:0")


def _regime(rows, T, ydt):
    """(RB, row blocks, launched workgroups) by the launcher's own arithmetic (gnode_l1_loss_scaled_f32)."""
    per_row = T * 3 * (8 if ydt == "float64" else 4)
    assert per_row <= LDS_CAP
    spread = max(4, -(-rows // LOSS_GRID))
    RB = max(1, min(64, spread, LDS_CAP // per_row))
    nblocks = -(-rows // RB)
    return RB, nblocks, min(LOSS_GRID, nblocks)


def _inputs(rows, T, ydt, dev, seed=0):
    """S, I, R [T, rows, 1] leaves and labels [rows, T, 3] with exact ties planted on every third row."""
    import torch
    gen = torch.Generator().manual_seed(T * 1000 + rows + seed)
    S, I, R = (torch.rand(T, rows, 1, generator=gen).to(dev).requires_grad_(True) for _ in range(3))
    y = torch.rand(rows, T, 3, generator=gen, dtype=getattr(torch, ydt)).to(dev)
    with torch.no_grad():
        y[::3, :, 0] = S[:, ::3, 0].T.to(y.dtype)                     # exact ties: sign 0, as torch's abs backward
    return S, I, R, y


def _torch_loss(S, I, R, y, t0):
    import torch
    pred = torch.cat((S, I, R), -1).transpose(0, 1)[:, t0:, :]
    return (pred.to(y.dtype) - y[:, t0:, :]).abs().double().sum()


def _check_against_torch(S, I, R, y, t0):
    import torch
    from gnode.autograd import l1_loss_sum
    want = _torch_loss(S, I, R, y, t0)
    gw = torch.autograd.grad(want * 0.37, (S, I, R))
    got = l1_loss_sum(S, I, R, y, t0)
    assert got.dtype == torch.float64 and abs(float(got.detach()) - float(want.detach())) <= 1e-12 * float(want.detach())
    gg = torch.autograd.grad(got * 0.37, (S, I, R))
    for a, b in zip(gg, gw):
        assert a.shape == b.shape and torch.equal(a, b.to(a.dtype))
    again = l1_loss_sum(S, I, R, y, t0)
    assert float(again.detach()) == float(got.detach())
    return got.detach()


# rows, T, labels, t0 | RB, row blocks, rows of the last block
@pytest.mark.parametrize("rows,T,ydt,t0,RB,nblocks,last", [
    (70001, 3, "float32", 1, 64, 1094, 49),       # the grid wraps (70 workgroups take a second block), ragged last block
    (66001, 2, "float64", 0, 64, 1032, 17),       # wrap with float64 labels, no grid point skipped
    (11, 700, "float64", 1, 2, 6, 1),             # the LDS cap decides RB (16 800 B per row: two fit), ragged
    (3, 2048, "float64", 1, 1, 3, 1),             # 48 KB of dynamic LDS exactly
    (3, 4096, "float32", 1, 1, 3, 1),             # the same through the float32 instantiation
])
def test_l1_loss_regimes_match_the_torch_expression(rows, T, ydt, t0, RB, nblocks, last, dev):
    assert _regime(rows, T, ydt) == (RB, nblocks, min(LOSS_GRID, nblocks))           # the regime this case is here for
    assert rows - (nblocks - 1) * RB == last
    if rows > 65536:
        assert nblocks > LOSS_GRID                                                   # a later kLossGrid must not lose the wrap
    if RB == 1:
        assert T * 3 * (8 if ydt == "float64" else 4) == LDS_CAP
    S, I, R, y = _inputs(rows, T, ydt, dev)
    _check_against_torch(S, I, R, y, t0)


def test_l1_loss_single_element(dev):
    S, I, R, y = _inputs(1, 1, "float32", dev)                        # row 0 carries a tie in S
    got = _check_against_torch(S, I, R, y, 0)
    want = abs(np.float32(I.item()) - np.float32(y[0, 0, 1].item())).astype(np.float64) + \
        abs(np.float32(R.item()) - np.float32(y[0, 0, 2].item())).astype(np.float64)
    assert float(got) == float(want)                                  # two terms: no summation order to speak of


@pytest.mark.parametrize("rows,T,ydt", [(7, 5, "float32"), (130, 3, "float64")])
def test_l1_loss_with_t0_equal_T_is_exactly_zero(rows, T, ydt, dev):
    """t0 = T leaves no grid point: the sum is +0.0 and every sign is 0 (the launcher admits t0 <= T)."""
    import torch
    from gnode import ops
    S, I, R, y = _inputs(rows, T, ydt, dev)
    total, sgn = ops.l1_loss_sum(S, I, R, y, T)
    assert float(total) == 0.0 and not np.signbit(float(total))
    assert tuple(sgn.shape) == (3, T, rows) and not sgn.any()
    got = _check_against_torch(S, I, R, y, T)                         # torch's empty slice sums to 0.0 as well
    assert float(got) == 0.0


@pytest.mark.parametrize("T,ydt", [(2049, "float64"), (4097, "float32")])
def test_l1_loss_label_row_past_the_lds_cap_raises(T, ydt, dev):
    """One label row more than 48 KB: refused, and the device serves the next call."""
    from gnode import ops
    from gnode._lib import GnodeError
    assert T * 3 * (8 if ydt == "float64" else 4) > LDS_CAP >= (T - 1) * 3 * (8 if ydt == "float64" else 4)
    S, I, R, y = _inputs(2, T, ydt, dev)
    with pytest.raises(GnodeError):
        ops.l1_loss_sum(S, I, R, y, 1)
    S, I, R, y = _inputs(5, 4, ydt, dev)
    _check_against_torch(S, I, R, y, 1)


@pytest.mark.parametrize("rows,T,ydt,t0", [(70001, 3, "float32", 1), (37, 6, "float64", 2)])
def test_l1_loss_mean_backward_writes_scaled_signs(rows, T, ydt, t0, dev):
    """l1_loss_mean_backward (the sign_scale argument of the kernel): the sum of l1_loss_sum, and S.grad, I.grad, R.grad
    = sign(pred - y) * float32(1 / count) exactly, 0 below t0 and on the planted ties."""
    import torch
    from gnode import ops
    from gnode.autograd import l1_loss_mean_backward, l1_loss_sum
    if rows > 65536:
        assert _regime(rows, T, ydt)[1] > LOSS_GRID
    S, I, R, y = _inputs(rows, T, ydt, dev)
    count = rows * (T - t0) * 3
    with torch.no_grad():
        plain = l1_loss_sum(S, I, R, y, t0)
    _, sgn = ops.l1_loss_sum(S, I, R, y, t0)                          # signs at scale 1: -1, 0, +1
    assert set(torch.unique(sgn).tolist()) == {-1.0, 0.0, 1.0}
    total = l1_loss_mean_backward(S, I, R, y, count, t0)
    assert total.dtype == torch.float64 and float(total) == float(plain)
    # the sign itself, from the torch expression in the labels' dtype
    pred = torch.cat((S, I, R), -1).detach().transpose(0, 1)                          # [rows, T, 3]
    want_sign = torch.sign(pred.to(y.dtype) - y).to(torch.float32)
    want_sign[:, :t0, :] = 0.0
    assert torch.equal(sgn.permute(2, 1, 0), want_sign)
    scale = np.float32(1.0 / count)
    for c, leaf in enumerate((S, I, R)):
        g = leaf.grad
        assert g is not None and g.shape == leaf.shape and g.dtype == torch.float32
        want = (want_sign[:, :, c].T.cpu().numpy() * scale).astype(np.float32)       # sign * float32(1 / count): exact in fp32
        assert np.array_equal(g[:, :, 0].cpu().numpy(), want)
        assert not g[:t0].any()                                                       # grid points below t0: exactly 0
    assert not S.grad[:, ::3, 0].any()                                                # the planted ties


@pytest.mark.parametrize("rows,T,ydt,t0", [(70001, 3, "float32", 1), (11, 700, "float64", 1), (5, 4, "float32", 0)])
def test_l1_loss_without_sign_returns_the_same_bits(rows, T, ydt, t0, dev):
    import torch
    from gnode import ops
    S, I, R, y = _inputs(rows, T, ydt, dev)
    with_sign, sgn = ops.l1_loss_sum(S, I, R, y, t0, want_sign=True)
    without, none = ops.l1_loss_sum(S, I, R, y, t0, want_sign=False)
    assert sgn is not None and none is None
    assert with_sign.dtype == without.dtype == torch.float64
    assert np.float64(float(with_sign)).tobytes() == np.float64(float(without)).tobytes()
