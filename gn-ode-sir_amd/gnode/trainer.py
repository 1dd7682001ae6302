"""Trainer plumbing around the hot path: what the reference's L3
scripts do around `model(x)` -- dataset assembly, splits, Adam/L1 loop, best-val -> test,
CSV rows -- restated as a library so the drop-in entry scripts stay thin.

    single graph : ode_nn_ngraph_sim.py:323-486   (monitorer-sim.py, model='ode_nn')
    multi graph  : ode_nn_ngraphs.py:291-415      (monitorer-ngraphs.py, model='ode_nn')

Differences that are deliberate (and invisible to the file/argv contract):
  * the row subsample of get_sir_t_nodes_torch (ode_nn.py:249-261) is fused into the
    forward (`out_rows`), and the loss is assembled on the GPU (no per-row D2H copies);
  * under torch.distributed (one process per GPU) every batch is sharded over ranks and
    the 4 809-float gradient is all-reduced once per optimiser step (RCCL over xGMI);
    with WORLD_SIZE=1 this is exactly the reference's single-device loop.
"""
from __future__ import annotations

import argparse
import csv
import os
import pickle
import time

import numpy as np
import torch
import torch.nn as nn

from . import ops, sharding
from .autograd import l1_loss_mean_backward, l1_loss_sum
from .ode_nn import _counts_f64, _device_graph_for, create_graph, sir_counts, sir_torch

# GNODE_ADJOINT=0 (read ONCE at import): the drop-in scripts build their ODEBlock with adjoint=False and train with the exact
# gradient of the Euler solve instead of the reference's adjoint gradient; argv is untouched.
ADJOINT_DEFAULT = os.environ.get("GNODE_ADJOINT", "1") != "0"


# --------------------------------------------------------------------------- CSV (ode_nn.py:374-392)
def csv_trials(path_to_csv, columns, list_to_csv):
    new = not os.path.exists(path_to_csv)
    with open(path_to_csv, "w" if new else "a+", newline="") as fh:
        w = csv.writer(fh)
        if new:
            w.writerow(columns)
        w.writerow(list_to_csv)


def save_trial_to_csv(args, best_epoch, val_loss, test_loss, loss_baseline, n_ode_time, rk_time):
    row = [args.trial, args.model, args.lr, args.epochs, args.sim, args.train_val_test_ratio, len(args.beta), len(args.gamma),
           args.deltaT, args.maxTime, [len(args.I_indices[0]), len(args.I_indices)], args.hidden, best_epoch, val_loss,
           test_loss, loss_baseline, n_ode_time, rk_time]
    csv_trials(args.path_to_save + "/Metrics-trials-" + os.path.relpath(args.dataset, "./real_graphs/"),
               ["trial", "model", "lr", "epochs", "MC sim", "train_val_test_ratio", "beta", "gamma", "deltaT", "maxTime",
                "I_indices", "hidden", "best_epoch", "val_loss", "test_loss", "loss_baseline", "n_ode_time", "rk_time"], row)


# --------------------------------------------------------------------------- labels (ode_nn_ngraph_sim.py:190-206)
def label_paths(dataset, path_to_save, I_indices):
    stem = path_to_save + "/" + dataset[14:] + "-{}-" + "-".join(str(i) for i in I_indices) + ".pkl"
    return [stem.format(c) for c in "SIR"]


def load_SIR_labels(dataset, path_to_save, G, I_indices, beta, gamma, sim, maxTime):
    """Label cache keyed by the seed set only (reference quirk Q4): load the three
    [T, n] probability arrays if present, else generate them with the Monte-Carlo kernel,
    divide the counts by `sim` (ode_nn_ngraph_sim.py:199) and write the same files.

    Under torch.distributed this is a COLLECTIVE: the `sim` trajectories are split over the ranks
    (coins are keyed by the global trajectory index), the uint32 [3,T,n] counts are all-reduced
    once per sample, and rank 0 writes the cache."""
    return _label_store(label_paths(dataset, path_to_save, I_indices), G, I_indices, beta, gamma, sim, maxTime, False)


def _label_store(ps, G, I_indices, beta, gamma, sim, maxTime, raw_counts):
    """Load-or-generate behind both label conventions.  raw_counts=False: files hold probabilities (single-graph
    script, ode_nn_ngraph_sim.py:190-206); raw_counts=True: files hold COUNTS and the loader divides by `sim`
    (the multi-graph script's wiki-vote convention, ode_nn_ngraphs.py:168-171).  Returns probabilities."""
    rank, world = sharding.world_info()
    have = os.path.exists(ps[0])
    coll = sharding.collectives_on()
    if coll:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        flag = torch.tensor([1 if have else 0], device=dev)
        torch.distributed.broadcast(flag, src=0)
        have = bool(flag.item())
    if have:
        out = tuple(pickle.load(open(p, "rb")) for p in ps)
        return tuple(a / sim for a in out) if raw_counts else out
    if not coll:
        S, I, R = sir_torch(G, I_indices, beta, gamma, sim, maxTime)
        cnt = (S[0], I[0], R[0])
    else:
        seed = torch.randint(0, 2**62, (1,), dtype=torch.int64).to(dev)
        torch.distributed.broadcast(seed, src=0)
        graph = _device_graph_for(G)
        lo, hi = sharding.shard_range(sim, rank, world)
        counts = sir_counts(graph, I_indices, beta, gamma, hi - lo, maxTime, int(seed.item()), sim_offset=lo)
        sharding.allreduce_counts(counts)
        cnt = tuple(_counts_f64(counts))
    out = tuple(a / sim for a in cnt)
    if rank == 0:
        for p, a in zip(ps, cnt if raw_counts else out):
            pickle.dump(a, open(p, "wb"))
    sharding.barrier()
    return out


def label_tensor(S, I, R) -> torch.Tensor:
    """Three [T, n] label arrays -> the sample's y [n, T, 3] float64, contiguous."""
    return torch.from_numpy(np.stack([np.asarray(S), np.asarray(I), np.asarray(R)], -1)).transpose(0, 1).contiguous()


def _graph_cache() -> bool:
    """GNODE_GRAPH_CACHE=1: create_graph keeps a CSR file next to each graph pickle."""
    return os.environ.get("GNODE_GRAPH_CACHE", "0") == "1"


def _decode_seeds(args):
    """--I_indices "[25, 18]" "[3, 7]" -> [[25, 18], [3, 7]], in place."""
    args.I_indices = [list(map(int, str(i)[1:-1].split(", "))) for i in args.I_indices]


def _save_initial(args):
    """The experiment's initial-{seed,beta,gamma}.pkl, unless they are there already."""
    if not os.path.exists(args.path_to_save + "/initial-seed.pkl"):
        for name, val in (("seed", args.I_indices), ("beta", args.beta), ("gamma", args.gamma)):
            pickle.dump(val, open(args.path_to_save + f"/initial-{name}.pkl", "wb"))


def _labels_of(args, G):
    """(S, I, R) of every sample of a single-graph experiment, loaded or generated in sample order."""
    return [load_SIR_labels(args.dataset, args.path_to_save, G, seeds, args.beta[i], args.gamma[i], args.sim, args.maxTime)
            for i, seeds in enumerate(args.I_indices)]


# --------------------------------------------------------------------------- dataset assembly
def sample_tensor(n_nodes, hidden, seeds, beta, gamma, marker=None):
    """x_i = [S0 | I0 | R0 | beta-gamma slab] in [n, 3+H] (ode_nn_ngraph_sim.py:373-390;
    multi-graph marker at slab column 2 of node 0, ode_nn_ngraphs.py:333)."""
    x = torch.zeros(n_nodes, 3 + hidden, dtype=torch.float32)
    x[:, 0] = 1.0
    x[list(seeds), 0] = 0.0
    x[list(seeds), 1] = 1.0
    x[:, 3] = beta
    x[:, 4] = gamma
    if marker is not None:
        x[0, 5] = marker
    return x


def split_indices(n_items, ratio, out_of_dist=None):
    """Sequential split by ratio (ode_nn_ngraph_sim.py:385-397) or by the index dict of
    out-of-dist-gamma.pkl (:399-414)."""
    if out_of_dist is not None:
        tr = [i for i in range(n_items) if i in out_of_dist["train"]]
        va = [i for i in range(n_items) if i in out_of_dist["val"]]
        te = [i for i in range(n_items) if i not in out_of_dist["train"] and i not in out_of_dist["val"]]
        return tr, va, te
    a = int(ratio[0] * n_items)
    b = int((ratio[0] + ratio[1]) * n_items)
    return list(range(0, a)), list(range(a, b)), list(range(b, n_items))


# --------------------------------------------------------------------------- epoch loops
class Runner:
    """model + optimiser + the epoch loops of the reference (train :208-270, test :272-296).

    `stack=True`: single-graph batches [B, n, 3+H] (DataLoader of ode_nn_ngraph_sim.py:416-429);
    `stack=False`: multi-graph batches concatenated along the node axis (ode_nn_ngraphs.py:179-196).
    Under torch.distributed every batch's samples are split into contiguous per-rank blocks; each
    rank back-propagates its share of the GLOBAL element-mean L1 (:234, :248-249) and the gradients
    are summed with one flat all-reduce."""

    def __init__(self, model, lr, maxTime, deltaT, device, stack, use_graphs=None):
        self.model, self.device, self.stack = model, device, stack
        # Launch-bound regime (the reference trains with batch_size 1 on small graphs): capture
        # forward + loss + adjoint backward of each batch shape ONCE into a HIP graph and replay it.
        # Single-graph batches only (the multi-graph forward reads its markers on the host).
        if use_graphs is None:
            use_graphs = os.environ.get("GNODE_TRAIN_GRAPHS", "1") != "0"
        self.on_gpu = torch.cuda.is_available() and str(device).startswith("cuda")
        self.use_graphs = bool(use_graphs) and stack and self.on_gpu
        self._graphs = {}
        self._marks, self._picks = {}, None
        # same Adam as the reference (:442); on the GPU the whole update is ONE kernel instead of ~16 tiny ones
        self.opt = torch.optim.Adam(model.parameters(), lr=lr, fused=True) if self.on_gpu else torch.optim.Adam(model.parameters(), lr=lr)
        self.rows = ops.subsample_rows(maxTime, deltaT)
        self.rank, self.world = sharding.world_info()
        self.collective = sharding.collectives_on()      # world > 1, or a forced single-rank rehearsal of the RCCL calls
        seed = torch.randint(0, 2**31 - 1, (1,))
        if self.collective:
            seed = seed.to(device)
            torch.distributed.broadcast(seed, src=0)
            for p in model.parameters():                 # every rank starts from rank 0's initialisation
                torch.distributed.broadcast(p.data, src=0)
        self.seed = int(seed.item())

    def place(self, *lists, budget_frac=0.5):
        """Keep the dataset resident in HBM when it fits (a 75k-node sample is 20 MB of x + 54 MB of float64
        labels; 288 GB holds thousands): the per-batch `.to(device)` of the reference's loop (:221-222) then
        moves nothing.  Falls back to host tensors (pageable H2D per batch) when it does not fit."""
        if not self.on_gpu:
            return lists
        need = sum(t.numel() * t.element_size() for l in lists for t in l)
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > budget_frac * free:
            return lists
        return tuple([t.to(self.device) for t in l] for l in lists)

    def batches(self, n_items, batch_size, shuffle, epoch=0):
        if shuffle and not self.stack:
            epoch = 0      # multi-graph: the reference shuffles ONCE, before the epoch loop (ode_nn_ngraphs.py:179-196, :359),
                           # and reuses those batches -- which also keeps the per-composition device graphs few and reusable
        if shuffle:
            g = torch.Generator().manual_seed(self.seed + epoch)       # same permutation on every rank
            idx = torch.randperm(n_items, generator=g).tolist()
        else:
            idx = list(range(n_items))
        return [idx[i:i + batch_size] for i in range(0, n_items, batch_size)]

    def _local(self, xs, ys, sel, as_lists=False):
        lo, hi = sharding.shard_range(len(sel), self.rank, self.world)
        mine = sel[lo:hi]
        if not mine:
            return None, None
        if as_lists:                                 # HIP-graph replay: the samples are copied straight into the graph's static inputs
            return [xs[j] for j in mine], [ys[j] for j in mine]
        x = torch.stack([xs[j] for j in mine]) if self.stack else torch.cat([xs[j] for j in mine], 0)
        y = torch.cat([ys[j] for j in mine], 0)
        # multi-graph batches: which graph each sample sits on (its marker, ode_nn_ngraphs.py:333) is read ONCE per sample, not
        # once per forward -- the batches are fixed and a host read-back per step keeps the host from running ahead
        self._picks = None if self.stack else tuple(self._mark(xs[j]) for j in mine)
        return x.to(self.device), y.to(self.device)

    def _mark(self, xj):
        m = self._marks.get(id(xj))
        if m is None or m[0] is not xj:
            m = (xj, int(xj[0, 3 + 2].item()) - 1)          # (the tensor is kept so that its id stays its own)
            self._marks[id(xj)] = m
        return m[1]

    def _model_out(self, x):
        """(S, I, R) at the label rows for the batch `_local` built last"""
        if not self.stack and self._picks:
            return self.model(x, out_rows=self.rows, picks=self._picks)
        return self.model(x, out_rows=self.rows)

    def _loss_sum(self, x, y):
        # L1 over cat(S, I, R)[rows, T, 3][:, 1:, :] (t = 0 excluded, :234) and its gradient: one kernel instead of the
        # cat / transpose / convert / subtract / abs / sum chain and its six backward launches
        return l1_loss_sum(*self._model_out(x), y, 1)

    def _loss_backward(self, x, y, gcount):
        """forward + loss + backward of one batch (gradients of the element-mean L1 over `gcount` elements); returns the loss sum"""
        return l1_loss_mean_backward(*self._model_out(x), y, gcount, 1)

    def _graphed_backward(self, x_list, y_list, gcount):
        """Replay (capturing on first use) forward + L1 + backward for this batch shape; returns the loss sum.  x_list / y_list:
        the batch's samples ([n, 3+H] / [n, T, 3] each); they are copied straight into the graph's static inputs (one copy per
        tensor: stacking first would be a second one)."""
        B, n = len(x_list), x_list[0].shape[0]
        key = (B, tuple(x_list[0].shape), tuple(y_list[0].shape), y_list[0].dtype, gcount)
        ent = self._graphs.get(key)

        def fill(xs, ys):
            for b in range(B):
                xs[b].copy_(x_list[b], non_blocking=True)
                ys[b * n:(b + 1) * n].copy_(y_list[b], non_blocking=True)

        if ent is None:
            xs = torch.zeros((B,) + tuple(x_list[0].shape), dtype=x_list[0].dtype, device=self.device)
            ys = torch.zeros((B * n,) + tuple(y_list[0].shape[1:]), dtype=y_list[0].dtype, device=self.device)
            fill(xs, ys)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                 # warm-up: sets kernel attributes, sizes the allocator's pools
                self._loss_backward(xs, ys, gcount)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            # the captured backward CREATES the gradient tensors (in the graph's pool: fixed addresses, rewritten by every
            # replay) instead of zero-filling and accumulating into existing ones -- 16 tiny launches less per step
            params = [p for p in self.model.parameters()]
            for p in params:
                p.grad = None
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ls_out = self._loss_backward(xs, ys, gcount).detach()
            ent = (graph, xs, ys, ls_out, [p.grad for p in params])
            self._graphs[key] = ent
        graph, xs, ys, ls_out, grads = ent
        fill(xs, ys)
        graph.replay()
        for p, g in zip(self.model.parameters(), grads):       # each batch shape's graph owns its gradient tensors
            p.grad = g
        return ls_out

    def train_epoch(self, xs, ys, batch_size, epoch):
        self.model.train()
        items, t_fwd = 0, 0.0
        # the epoch's loss sum stays on the device: one host sync per EPOCH, not one per optimiser step, so the host
        # runs ahead and the launch-bound small configurations are not throttled by a D2H read-back every step
        tot_t = torch.zeros((), dtype=torch.float64, device=self.device)
        T = ys[0].shape[1] if ys else 0
        for sel in self.batches(len(xs), batch_size, True, epoch):
            gcount = sum(ys[j].shape[0] for j in sel) * (T - 1) * 3       # elements of the GLOBAL batch
            x, y = self._local(xs, ys, sel, as_lists=self.use_graphs)
            if not self.use_graphs:
                self.opt.zero_grad(set_to_none=True)
            elif x is None:
                self.opt.zero_grad(set_to_none=False)                     # (a replay rewrites the gradients; nothing does for a rank without samples)
            if x is not None and self.use_graphs:
                t0 = time.time()
                tot_t += self._graphed_backward(x, y, gcount).to(torch.float64)   # grads are (re)written by the replay
                t_fwd += time.time() - t0
            elif x is not None:
                t0 = time.time()
                ls = self._loss_backward(x, y, gcount)
                t_fwd += time.time() - t0
                tot_t += ls.detach().to(torch.float64)
            if self.collective:
                for p in self.model.parameters():                        # ranks without samples contribute zeros
                    if p.grad is None and p.requires_grad:
                        p.grad = torch.zeros_like(p)
                sharding.allreduce_flat_grads([p for p in self.model.parameters() if p.grad is not None])
            self.opt.step()
            items += gcount
        if self.collective:
            torch.distributed.all_reduce(tot_t)
        self._check_launches()
        return float(tot_t) / max(items, 1), t_fwd

    def _check_launches(self):
        """Once per epoch (there is a host sync here anyway): did a persistent launch give up waiting for its group?  Its spins
        are bounded so that a lost workgroup becomes this error instead of a hang (csrc/gnode_pers64.hip, gnode_persg.hip)."""
        if not self.on_gpu:
            return
        f, b = ops.forward_status(), ops.backward_status()
        if f or b:
            raise RuntimeError(f"a persistent launch gave up (forward code {f}, backward code {b}): its outputs are invalid -- "
                               "is another process using this GPU?  GNODE_PERSIST=0 runs one launch per step")

    @torch.no_grad()
    def evaluate(self, xs, ys, batch_size):
        self.model.eval()
        sums, counts = [], []
        T = ys[0].shape[1] if ys else 0
        for sel in self.batches(len(xs), batch_size, False):
            gcount = sum(ys[j].shape[0] for j in sel) * (T - 1) * 3
            x, y = self._local(xs, ys, sel)
            sums.append(self._loss_sum(x, y).to(torch.float64) if x is not None
                        else torch.zeros((), dtype=torch.float64, device=self.device))
            counts.append(gcount)
        if not sums:
            return 0.0, []
        allsum = torch.stack(sums)                                   # one read-back for the whole pass
        if self.collective:
            torch.distributed.all_reduce(allsum)
        vals = allsum.cpu().tolist()
        self._check_launches()
        per_batch = [v / max(c, 1) for v, c in zip(vals, counts)]
        return sum(vals) / max(sum(counts), 1), per_batch

    def fit(self, train, val, test, epochs, batch_size, test_batch_size):
        """The reference's epoch loop (ode_nn_ngraph_sim.py:444-470, ode_nn_ngraphs.py:380-402) over (xs, ys) pairs: train, validate,
        and on every best validation loss evaluate the test set.  Returns (best_epoch, best val loss, test loss, per-batch test
        losses, seconds of that test pass)."""
        best_loss, best_epoch, test_loss, test_all, t_test = np.inf, -1, float("nan"), [], 0.0
        print("training...")
        for epoch in range(epochs):
            loss, t_fwd = self.train_epoch(*train, batch_size, epoch)
            val_loss, _ = self.evaluate(*val, batch_size)
            print("Time: ", t_fwd)
            print("Epoch: {:03d}, Train Loss: {:.10f}, Val Loss: {:.10f}".format(epoch, loss, val_loss))
            if val_loss < best_loss:
                best_loss, best_epoch = val_loss, epoch
                t0 = time.time()
                test_loss, test_all = self.evaluate(*test, test_batch_size)
                t_test = time.time() - t0
        return best_epoch, best_loss, test_loss, test_all, t_test


# --------------------------------------------------------------------------- single-graph entry (ode_nn_ngraph_sim.py:323-486)
def parser_single():
    p = argparse.ArgumentParser(description="Neural ODE")
    p.add_argument("--lr", type=float, default=1e-2)
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--sim", type=int, default=1000)
    p.add_argument("--beta", type=float, nargs="+", default=[0.2])
    p.add_argument("--gamma", type=float, nargs="+", default=[0.1])
    p.add_argument("--deltaT", type=float, default=0.5)
    p.add_argument("--maxTime", type=int, default=20)
    p.add_argument("--I_indices", nargs="+", default=[12])
    p.add_argument("--hidden", type=int, default=32)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--path_to_save", default="./plots")
    p.add_argument("--trial", type=int, default=32)
    p.add_argument("--dataset", default="none")
    p.add_argument("--train_val_test_ratio", nargs=3, type=float, default=[5e-1, 1e-1, 4e-1])
    p.add_argument("--model", default="ode_nn", type=str)
    p.add_argument("--out_of_dist", default=False, action="store_true")
    return p


def main_single(argv=None):
    from .ode_nn_ngraph_sim import ODEBlock, ODEfunc
    args = parser_single().parse_args(argv)
    if args.model != "ode_nn":
        raise SystemExit(f"this entry point serves model='ode_nn' only (got {args.model!r})")
    rank, world = sharding.init_from_env()        # torchrun: one process per GPU; plain run: (0, 1)
    G, A, _ = create_graph(50, args.dataset, cache=_graph_cache())
    n_nodes = A.shape[0]
    print(n_nodes)
    _decode_seeds(args)
    if rank == 0:
        _save_initial(args)
    xs = [sample_tensor(n_nodes, args.hidden, seeds, args.beta[i], args.gamma[i]) for i, seeds in enumerate(args.I_indices)]
    ys = [label_tensor(*lab) for lab in _labels_of(args, G)]
    ood = pickle.load(open(args.path_to_save + "/out-of-dist-gamma.pkl", "rb")) if args.out_of_dist else None
    tr, va, te = split_indices(len(xs), args.train_val_test_ratio, ood)
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    torch.set_default_dtype(torch.float32)
    print(device)
    odefunc = ODEfunc(A, args.beta[0], args.gamma[0], args.hidden, device)
    model = ODEBlock(args.maxTime, args.deltaT, n_nodes, args.I_indices[0], args.hidden, odefunc, device,
                     adjoint=ADJOINT_DEFAULT).to(device)
    run = Runner(model, args.lr, args.maxTime, args.deltaT, device, stack=True)
    xs, ys = run.place(xs, ys)
    pick = lambda ids: ([xs[i] for i in ids], [ys[i] for i in ids])
    best_epoch, best_loss, test_loss, test_all, t_test = run.fit(pick(tr), pick(va), pick(te), args.epochs, args.batch_size, 1)
    if rank != 0:
        return 0
    if not args.out_of_dist:
        # the reference leaves the mean-field comparison switched off (ode_nn_ngraph_sim.py:473-474: zeros in the CSV);
        # GNODE_RK_BASELINE=1 fills the two columns with `runge_kutta_baseline` (:298-317) on the test samples
        loss_baseline, rk_time = 0, 0
        if os.environ.get("GNODE_RK_BASELINE", "0") == "1":
            loss_baseline, rk_time = runge_kutta_baseline(A, args, te, ys)
        save_trial_to_csv(args, best_epoch, best_loss, test_loss, loss_baseline, t_test, rk_time)
    else:
        rel = os.path.relpath(args.dataset, "./real_graphs/")
        csv_trials(args.path_to_save + "/Out-of-dist-gamma-" + rel, [str(i) for i in ood["test"]], test_all)
        csv_trials(args.path_to_save + "/Out-of-dist-gamma-trials-" + rel,
                   ["trial", "model", "lr", "epochs", "deltaT", "maxTime", "hidden", "best_epoch", "val_loss", "test_loss", "n_ode_time"],
                   [args.trial, args.model, args.lr, args.epochs, args.deltaT, args.maxTime, args.hidden, best_epoch, best_loss,
                    test_loss, t_test])
    return 0


def runge_kutta_baseline(A, args, test_ids, ys):
    """reference ode_nn_ngraph_sim.py:298-317: mean of the three per-compartment MAEs of the mean-field solution
    against the Monte-Carlo labels, averaged over the test samples; returns (loss, seconds)."""
    from .ode_nn import runge_kutta_order4, sir
    t0, losses = time.time(), []
    for i in test_ids:
        I_t, S_t, R_t = runge_kutta_order4(sir, A, A.shape[0], args.I_indices[i], args.beta[i], args.gamma[i], args.deltaT,
                                           args.maxTime)
        y = ys[i].cpu().numpy()                                   # [n, T, 3]
        losses.append((np.abs(S_t - y[:, :, 0].T).mean() + np.abs(I_t - y[:, :, 1].T).mean() +
                       np.abs(R_t - y[:, :, 2].T).mean()) / 3)
    dt = time.time() - t0
    print("Runge-kutta baseline Loss: {:.5f}".format(float(np.mean(losses))))
    print("Time inference baseline: {:.5f}".format(dt))
    return float(np.mean(losses)), dt


# --------------------------------------------------------------------------- DMP comparison entry (dmp.py:212-375)
def main_dmp(argv=None):
    """What monitorer-sim.py spawns for model='dmp' (monitorer-sim.py:30-31): same argv and label / initial-* files
    as the single-graph script; runs `DMP_SIR(A*beta, [gamma]*n).run(seeds, maxTime)` on every test sample and
    prints the element-weighted L1 against the Monte-Carlo labels (dmp.py:345-364; the reference saves nothing).
    The samples go through `dmp_batch` in chunks of at most 64 on one graph handle: each sample's bits, and so every
    printed loss, are its solo `DMP_SIR` run's."""
    from .dmp import DmpGraph, dmp_batch
    args = parser_single().parse_args(argv)
    G, A, _ = create_graph(50, args.dataset, cache=_graph_cache())
    n_nodes = A.shape[0]
    print(n_nodes)
    _decode_seeds(args)
    _save_initial(args)                                           # (this script runs on its own: no ranks)
    ys = [np.stack([np.asarray(a) for a in lab], -1) for lab in _labels_of(args, G)]        # [T, n, 3]
    ood = pickle.load(open(args.path_to_save + "/out-of-dist-gamma.pkl", "rb")) if args.out_of_dist else None
    _, _, te = split_indices(len(ys), args.train_val_test_ratio, ood)
    import scipy.sparse as sp
    A1 = sp.csr_matrix(A).astype(np.float64)
    A1.data[:] = 1.0                                              # the reference multiplies the 0/1 adjacency by beta (:349)
    graph = DmpGraph(A1)
    te = list(te)
    t0, loss_all, items = time.time(), 0.0, 0
    for c0 in range(0, len(te), 64):
        chunk = te[c0:c0 + 64]
        gam = np.repeat(np.asarray([args.gamma[i] for i in chunk], dtype=np.float64)[:, None], n_nodes, axis=1)
        outs = dmp_batch(graph, [args.I_indices[i] for i in chunk], gam, args.maxTime,
                         scale=[args.beta[i] for i in chunk]).cpu().numpy()
        for i, out in zip(chunk, outs):
            print("dmp")
            loss = float(np.abs(out[1:].astype(np.float64) - ys[i][1:]).mean())
            cnt = 3 * n_nodes * (args.maxTime - 1)
            loss_all += loss * cnt
            items += cnt
            print(loss)
    test_loss = loss_all / max(items, 1)
    print("DMP baseline Loss: {:.5f}".format(test_loss))
    print("Time inference baseline: {:.5f}".format(time.time() - t0))
    return 0


# --------------------------------------------------------------------------- multi-graph entry (ode_nn_ngraphs.py:291-415)
def parser_multi():
    p = argparse.ArgumentParser(description="Neural ODE")
    p.add_argument("--lr", type=float, default=1e-2)
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--sim", type=int, default=1000)
    p.add_argument("--deltaT", type=float, default=0.5)
    p.add_argument("--maxTime", type=int, default=20)
    p.add_argument("--hidden", type=int, default=32)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--path_to_save", default="./plots")
    p.add_argument("--trial", type=int, default=32)
    p.add_argument("--dataset", default="none")
    p.add_argument("--train_val_test_ratio", nargs=3, type=float, default=[5e-1, 1e-1, 4e-1])
    p.add_argument("--model", default="ode_nn", type=str)
    p.add_argument("--instances_per_graph", type=int, nargs="+", default=[36, 36, 36, 36, 36, 120],
                   help="extension: the reference hard-codes this list (ode_nn_ngraphs.py:311)")
    p.add_argument("--standin", type=int, nargs=2, default=[75000, 500000], metavar=("N", "M"),
                   help="extension: nodes / undirected edges of the Erdos-Renyi stand-in used for a graph pickle that is "
                        "missing (the reference does not ship epinions.pkl)")
    p.add_argument("--per_sample_seeds", action="store_true",
                   help="extension: use each sample's own seed set; the reference infects ALL sampled seeds of a graph "
                        "in every sample (quirk Q5, ode_nn_ngraphs.py:343), which stays the default")
    return p


def load_multi_labels(dataset, path_to_save, I_indices, sim, G=None, beta=None, gamma=None, maxTime=None):
    """ode_nn_ngraphs.py:167-177 reads label files only (wiki-vote's hold raw counts, divided by `sim` on load) and the
    reference ships karate's alone.  Extension: a missing label set is generated with the
    Monte-Carlo kernel -- sharded over the ranks like the single-graph script's -- and written under the same names
    and conventions, so a clean experiment directory works."""
    stem = path_to_save + "/" + dataset + "-{}-" + "-".join(str(i) for i in I_indices) + ".pkl"
    ps = [stem.format(c) for c in "SIR"]
    if G is None and not os.path.exists(ps[0]):
        raise FileNotFoundError(ps[0])
    return _label_store(ps, G, I_indices, beta, gamma, sim, maxTime, raw_counts=(dataset == "wiki-vote"))


def standin_graph(name, n, m, seed=0):
    """Synthetic stand-in for a graph pickle the reference does not ship (`epinions.pkl`, .MISSING_LARGE_BLOBS):
    Erdos-Renyi G(n, m) with the node / edge counts asked for.  Returns (G, A, 0) like create_graph."""
    import scipy.sparse as sp
    from . import synth
    from .ode_nn import CsrGraph
    rp, ci = synth.er_csr(n, m, seed=seed)
    A = sp.csr_matrix((np.ones(ci.shape[0], dtype=np.int64), ci, rp), shape=(n, n))
    coo = sp.triu(A, k=1).tocoo()
    print(f"[gnode] {name}.pkl is not there: using a synthetic Erdos-Renyi stand-in G({n}, {m})")
    return CsrGraph(n, np.stack([coo.row, coo.col], 1)), A, 0


def ensure_initial_files(d, n_nodes, count, n_seeds):
    """`initial-{seed,beta,gamma}.pkl` of an experiment directory (written by monitorer-sim.py:209-226 runs in the
    reference's workflow): when absent, sample them as random_parameters_SIR does (monitorer-sim.py:105-121) --
    `n_seeds` distinct seed nodes, beta and gamma ~ U(0.1, 0.5) per sample -- on rank 0, and write them."""
    rank, _ = sharding.world_info()
    if rank == 0 and not os.path.exists(d + "/initial-seed.pkl"):
        os.makedirs(d, exist_ok=True)
        seeds = [[int(v) for v in np.random.choice(n_nodes, n_seeds, replace=False)] for _ in range(count)]
        pickle.dump(seeds, open(d + "/initial-seed.pkl", "wb"))
        pickle.dump([float(np.random.uniform(0.1, 0.5)) for _ in range(count)], open(d + "/initial-beta.pkl", "wb"))
        pickle.dump([float(np.random.uniform(0.1, 0.5)) for _ in range(count)], open(d + "/initial-gamma.pkl", "wb"))
    sharding.barrier()


def main_multi(argv=None):
    import networkx as nx
    from .ode_nn_ngraphs import ODEBlock, ODEfunc
    args = parser_multi().parse_args(argv)
    if args.model != "ode_nn":
        raise SystemExit(f"this entry point serves model='ode_nn' only (got {args.model!r})")
    rank, world = sharding.init_from_env()
    names = args.dataset[14:].split("+")
    A_list, G_list = [], []
    for gname in names:                                             # create_graphs, ode_nn_ngraphs.py:154-165
        label = args.dataset[:14] + gname
        if os.path.exists(label + ".pkl"):
            G, A, _ = create_graph(0, label, cache=_graph_cache())
        else:
            G, A, _ = standin_graph(gname, args.standin[0], args.standin[1])
        A_list.append(A)
        G_list.append(G)
    print(len(A_list))
    ipg = args.instances_per_graph
    n_train_graphs = len(ipg) - 2
    val_len = int(ipg[-1] / 2)
    tr, va, te = ([], []), ([], []), ([], [])
    count_val = 0
    for gi, gname in enumerate(names):
        if gname == "wiki-vote":
            path_load = "./multi-graph-1/Experiments-gpu-seed2"
        elif gname == "enron":
            path_load = "./multi-graph-1/Experiments2-seed2"
        else:
            last = args.path_to_save.split("/")[-1].split("-")
            path_load = "./multi-graph-1/" + last[0] + "-" + last[1]
        d = path_load + "-" + gname
        n_nodes = A_list[gi].shape[0]
        digits = "".join(ch for ch in path_load.split("seed")[-1] if ch.isdigit())       # "...-seed2" -> 2 seeds per sample
        ensure_initial_files(d, n_nodes, ipg[gi], int(digits) if digits else 2)
        I_all = pickle.load(open(d + "/initial-seed.pkl", "rb"))[:ipg[gi]]
        betas = pickle.load(open(d + "/initial-beta.pkl", "rb"))[:ipg[gi]]
        gammas = pickle.load(open(d + "/initial-gamma.pkl", "rb"))[:ipg[gi]]
        for i, indices in enumerate(I_all):
            S, I, R = load_multi_labels(gname, d, indices, args.sim, G_list[gi], betas[i], gammas[i], args.maxTime)
            y = label_tensor(S, I, R)
            seeds = indices if args.per_sample_seeds else [s for grp in I_all for s in (grp if isinstance(grp, (list, tuple)) else [grp])]
            x = sample_tensor(n_nodes, args.hidden, seeds, betas[i], gammas[i], marker=gi + 1)
            if gi <= n_train_graphs:
                dst = tr
            elif count_val < val_len:
                dst = va
                count_val += 1
            else:
                dst = te
            dst[0].append(x)
            dst[1].append(y)
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    torch.set_default_dtype(torch.float32)
    print(device)
    odefunc = ODEfunc(A_list, args.hidden, device)
    model = ODEBlock(args.maxTime, args.deltaT, args.hidden, odefunc, device, adjoint=ADJOINT_DEFAULT).to(device)
    run = Runner(model, args.lr, args.maxTime, args.deltaT, device, stack=False)
    tr, va, te = (run.place(*d) for d in (tr, va, te))
    best_epoch, best_loss, test_loss, _, t_test = run.fit(tr, va, te, args.epochs, args.batch_size, args.batch_size)
    if rank != 0:
        return 0
    csv_trials(args.path_to_save + "/Metrics-trials-" + os.path.relpath(args.dataset, "./real_graphs/"),
               ["trial", "model", "lr", "epochs", "deltaT", "maxTime", "hidden", "best_epoch", "val_loss", "test_loss", "n_ode_time"],
               [args.trial, args.model, args.lr, args.epochs, args.deltaT, args.maxTime, args.hidden, best_epoch, best_loss,
                test_loss, t_test])
    return 0
