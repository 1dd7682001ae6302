"""k_step64 deals a workgroup's first two tiles statically and draws every further tile from its queue's counter
(csrc/gnode_h64.hip).  Which workgroup visits a tile must change no bit: a batch through the multi-tile kernel is compared
BIT FOR BIT, sample by sample, with the same samples run one at a time, where every workgroup has a single tile and no
counter is read (the latency-mode instance).  Shapes: n = 3 001 (188 tiles per sample, the last one partial); 8 samples
-- fewer than two tiles per workgroup, every draw lands past the queue's end; 12 -- queue boundaries inside samples; 16 and
24 -- two and three samples per queue, most tiles drawn; rows with fewer than 8, more than 16 and (hub graph) more than 96
neighbours.  Parity with the reference itself is held by test_gpu_parity.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, BMAX = 3001, 19500, 24
DTS = np.asarray([0.5, 0.25, 1.0, 0.5, 0.125, 0.5, 0.5, 0.75, 0.25, 0.5, 1.0, 0.5], dtype=np.float32)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _graph(tail, dev):
    import torch
    from gnode import synth
    from gnode.graph import DeviceGraph
    rp, ci = synth.heavy_tail_csr(N, M, tail, seed=11) if tail else synth.er_csr(N, M, seed=11)
    deg = np.diff(rp)
    assert deg.min() < 8 and deg.max() > 16 and (not tail or deg.max() > 96), (deg.min(), deg.max())
    P = {k: torch.from_numpy(v).to(dev) for k, v in synth.linear_params(64, seed=12).items()}
    x = torch.from_numpy(synth.samples(N, BMAX, 64, seed=13)).to(dev)          # [BMAX, N, 67]
    return DeviceGraph(rp, ci), P, x


def _singles(g, P, x, B):
    """Every sample alone, one launch per step: [n_out, B * N] each, computed once per graph and left unchanged."""
    import torch
    from gnode import ops
    outs = [ops.forward(g, x[b].reshape(N, 67), P, DTS, "euler", None, persist=False)[:3] for b in range(B)]
    return [torch.cat([o[j] for o in outs], 1) for j in range(3)]


@pytest.fixture(scope="module")
def er(dev):
    g, P, x = _graph(0.0, dev)
    return g, P, x, _singles(g, P, x, BMAX)


@pytest.fixture(scope="module")
def hub(dev):
    g, P, x = _graph(0.8, dev)
    return g, P, x, _singles(g, P, x, 16)


def _check(case, B, repeats=1):
    import torch
    from gnode import _lib, ops
    g, P, x, ref = case
    xb = x[:B].reshape(B * N, 67)
    assert ops.forward_path(g, B * N, 64, len(DTS))[0] == 0          # too many rows for the persistent launch
    ws = torch.empty(_lib.load().gnode_forward_workspace_bytes(g.handle, B * N, 64, 0), dtype=torch.uint8, device=xb.device)
    for _ in range(repeats):                                         # again into the same workspace: counters start from zero
        got = ops.forward(g, xb, P, DTS, "euler", None, False, ws)[:3]
        assert ops.forward_status() == 0
        for a, b in zip(got, ref):
            assert torch.equal(a, b[:, :B * N]), float((a - b[:, :B * N]).abs().max())


@pytest.mark.parametrize("B", [8, 12, 16, 24])
def test_batch_equals_single_samples(B, er):
    _check(er, B, repeats=2 if B == 16 else 1)


def test_odd_then_even_step_count_same_workspace(er):
    """The counters alternate between two sets by step parity; a forward that ends on either set leaves the next one clean."""
    import torch
    from gnode import _lib, ops
    g, P, x, ref = er
    B = 16
    xb = x[:B].reshape(B * N, 67)
    ws = torch.empty(_lib.load().gnode_forward_workspace_bytes(g.handle, B * N, 64, 0), dtype=torch.uint8, device=xb.device)
    last = np.asarray([11], dtype=np.int32)
    a11 = ops.forward(g, xb, P, DTS[:11], "euler", last, False, ws)[0].clone()
    b12 = ops.forward(g, xb, P, DTS, "euler", None, False, ws)[0].clone()
    a11_again = ops.forward(g, xb, P, DTS[:11], "euler", last, False, ws)[0]
    assert torch.equal(b12, ref[0][:, :B * N]) and torch.equal(b12[11:12], a11) and torch.equal(a11, a11_again)


def test_hub_graph_batch_equals_single_samples(hub):
    _check(hub, 16)


def test_training_instance_batch_equals_single_samples(er):
    """want_sol: the instance that carries full Y_R rows and keeps the neighbour sums (three workgroups per CU)."""
    import torch
    from gnode import ops
    g, P, x, _ = er
    B, dts = 12, DTS[:5]
    S, I, R, sol = ops.forward(g, x[:B].reshape(B * N, 67), P, dts, "euler", None, True, want_keep=False, persist=False)
    sol = sol.reshape(len(dts) + 1, 4, B, N, 64)
    for b in range(B):
        s, i, r, so = ops.forward(g, x[b].reshape(N, 67), P, dts, "euler", None, True, want_keep=False, persist=False)
        for a, c in ((S, s), (I, i), (R, r)):
            assert torch.equal(a[:, b * N:(b + 1) * N], c), b
        so = so.reshape(len(dts) + 1, 4, N, 64)
        assert torch.equal(sol[:, :3, b], so[:, :3]), b              # the trajectory
        assert torch.equal(sol[:-1, 3, b], so[:-1, 3]), b            # beta / gamma at point 0, then the kept neighbour sums
