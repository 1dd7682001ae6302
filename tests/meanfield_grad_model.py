"""CPU model of the differentiable mean-field (a helper, not a test): the Dormand-Prince 5(4) solve of

    dS_v = -beta_v S_v ai_v,   dI_v = -dS_v - gamma_v I_v,   dR_v = gamma_v I_v,   ai_v = sum_{p in row v} w[rev p] I[col p]

for B samples on one graph, in a dtype given as a parameter (float64, or np.longdouble as the yardstick of float64's rounding).

    dp5_replay(...)       the forward from a given list of accepted steps
    dp5_replay_grad(...)  its exact reverse: the gradient of sum(gI * I + gS * S + gR * R) with the steps held fixed
    dp5_adaptive(...)     a restatement of the library's host controller, so that CPU tests have step lists of their own

States are [B, n] arrays S, I, R; beta and gamma are [B, n]; w is [nnz] in CSR position order (source = row, target = column)
or None = 1; beta None = 1.  Edge sums are np.add.at over the CSR positions, which works in every dtype.  Outputs are
[n_out, B, n]; a step list is (h [n_h], n_acc [n_out]) as gnode_meanfield_rates_steps_f64 records it."""
import numpy as np

A = [[],
     ["1/5"],
     ["3/40", "9/40"],
     ["44/45", "-56/15", "32/9"],
     ["19372/6561", "-25360/2187", "64448/6561", "-212/729"],
     ["9017/3168", "-355/33", "46732/5247", "49/176", "-5103/18656"],
     ["35/384", "0", "500/1113", "125/192", "-2187/6784", "11/84"]]
B4 = ["5179/57600", "0", "7571/16695", "393/640", "-92097/339200", "187/2100", "1/40"]


def _frac(s, dtype):
    p, _, q = s.partition("/")
    return dtype(int(p)) / dtype(int(q or 1))


def tableau(dtype):
    return [[_frac(x, dtype) for x in row] for row in A], [_frac(x, dtype) for x in B4]


def tables(rowptr, col):
    """(src, rev) of a symmetric pattern: the row of every CSR position and the position of its opposite entry"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = len(rowptr) - 1
    src = np.repeat(np.arange(n), np.diff(rowptr))
    pos = {(int(u), int(v)): p for p, (u, v) in enumerate(zip(src, col))}
    rev = np.array([pos[(int(v), int(u))] for u, v in zip(src, col)], np.int64).reshape(-1)
    return src, rev


class Problem:
    """One graph and one set of rates in `dtype`; f and its vector-Jacobian product."""

    def __init__(self, rowptr, col, beta, gamma, w, dtype=np.float64):
        self.dtype = dtype
        self.col = np.asarray(col, np.int64)
        self.src, self.rev = tables(rowptr, col)
        self.gamma = np.asarray(gamma, dtype)
        self.B, self.n = self.gamma.shape
        self.beta = np.ones((self.B, self.n), dtype) if beta is None else np.asarray(beta, dtype)
        self.w = np.ones(len(self.col), dtype) if w is None else np.asarray(w, dtype)
        self.w_in = self.w[self.rev] if len(self.col) else self.w

    def ai(self, I):
        out = np.zeros((self.B, self.n), self.dtype)
        if len(self.col):
            np.add.at(out, (slice(None), self.src), self.w_in[None, :] * I[:, self.col])     # ascending position within a row
        return out

    def f(self, Y):
        S, I, _ = Y
        inf = self.beta * (self.ai(I) * S)
        rec = self.gamma * I
        return (-inf, inf - rec, rec)

    def vjp(self, Y, kb, grads):
        """(Sbar, Ibar, Rbar) = kb^T df/dY at Y; adds this stage's share to grads = dict(beta, gamma, w [B, nnz])"""
        S, I, _ = Y
        kS, kI, kR = kb
        ai = self.ai(I)
        d, e = kI - kS, kR - kI
        c = d * self.beta * S
        Ibar = e * self.gamma
        if len(self.col):
            g = np.zeros((self.B, self.n), self.dtype)
            np.add.at(g, (slice(None), self.src), self.w[None, :] * c[:, self.col])           # row v: sum_q w[q] c[col q]
            Ibar = Ibar + g
            grads["w"] += c[:, self.col] * I[:, self.src]                                     # wbar[b][q] = c[col q] I[src q]
        grads["beta"] += d * ai * S
        grads["gamma"] += e * I
        return (d * self.beta * ai, Ibar, np.zeros_like(S))


def _stages(P, y, h, a):
    """Y_1 .. Y_7 of one step (Y_7 is the step's result) and k_1 .. k_6"""
    Y, K = [y], []
    for s in range(1, 7):
        K.append(P.f(Y[-1]))
        Y.append(tuple(y[c] + h * sum((a[s][j] * K[j][c] for j in range(s)), P.dtype(0)) for c in range(3)))
    return Y, K


def _state(init, dtype):
    init = np.asarray(init, dtype)
    return (init[:, :, 0].copy(), init[:, :, 1].copy(), init[:, :, 2].copy())


def dp5_replay(rowptr, col, init, beta, gamma, w, n_out, h, n_acc, dtype=np.float64, keep=False):
    """(I, S, R), [n_out, B, n] in `dtype`, from init [B, n, 3] and the steps (h, n_acc); keep: also every step's start state"""
    P = Problem(rowptr, col, beta, gamma, w, dtype)
    a, _ = tableau(dtype)
    y = _state(init, dtype)
    outs, kept, at = [y], [], 0
    for to in range(1, n_out):
        for i in range(int(n_acc[to])):
            kept.append(y)
            y = _stages(P, y, dtype(h[at + i]), a)[0][6]
        at += int(n_acc[to])
        outs.append(y)
    res = tuple(np.stack([o[c] for o in outs]) for c in (1, 0, 2))
    return (res, kept, P) if keep else res


def dp5_replay_grad(rowptr, col, init, beta, gamma, w, n_out, h, n_acc, gI, gS, gR, dtype=np.float64):
    """dict(init [B, n, 3], beta [B, n], gamma [B, n], w [B, nnz]): the gradient of sum(gI * I + gS * S + gR * R) of
    `dp5_replay`'s outputs, steps held fixed; gI, gS, gR are [n_out, B, n]"""
    (_, kept, P) = dp5_replay(rowptr, col, init, beta, gamma, w, n_out, h, n_acc, dtype, keep=True)
    a, _ = tableau(dtype)
    g = [np.asarray(x, dtype) for x in (gS, gI, gR)]
    grads = {"beta": np.zeros((P.B, P.n), dtype), "gamma": np.zeros((P.B, P.n), dtype), "w": np.zeros((P.B, len(P.col)), dtype)}
    yb = tuple(np.zeros((P.B, P.n), dtype) for _ in range(3))
    at = len(kept)
    for to in range(n_out - 1, 0, -1):
        yb = tuple(yb[c] + g[c][to] for c in range(3))
        for i in range(int(n_acc[to]) - 1, -1, -1):
            at -= 1
            hh = dtype(h[at])
            Y, _ = _stages(P, kept[at], hh, a)
            Yb = {7: yb}
            for s in range(6, 0, -1):                               # kbar_s = h sum_{t > s} a_ts Ybar_t, t from 7 down
                kb = tuple(sum(((hh * a[t - 1][s - 1]) * Yb[t][c] for t in range(7, s, -1)), dtype(0)) for c in range(3))
                Yb[s] = P.vjp(Y[s - 1], kb, grads)
            yb = tuple(sum((Yb[s][c] for s in range(6, 0, -1)), Yb[7][c]) for c in range(3))
    yb = tuple(yb[c] + g[c][0] for c in range(3))
    grads["init"] = np.stack(yb, axis=-1)
    return grads


def dp5_adaptive(rowptr, col, init, beta, gamma, w, t_out, rtol=1e-10, atol=1e-12, dtype=np.float64):
    """The library's host controller restated: ((I, S, R), h, n_acc, attempted steps).  First step 1e-3, steps clipped to the
    output times, error norm max |h sum_j (b_j - b4_j) k_j| / (atol + rtol max(|y|, |y'|)) over every sample, accept at <= 1,
    factor min(5, max(0.2, 0.9 err^-0.2))."""
    P = Problem(rowptr, col, beta, gamma, w, dtype)
    a, b4 = tableau(dtype)
    ecoef = [(a[6][j] if j < 6 else dtype(0)) - b4[j] for j in range(7)]
    y = _state(init, dtype)
    outs, hs, n_acc = [y], [], np.zeros(len(t_out), np.int32)
    t, h, steps = dtype(0), dtype(1e-3), 0
    for to in range(1, len(t_out)):
        t_end = dtype(t_out[to])
        while t < t_end:
            hh = min(h, t_end - t)
            Y, K = _stages(P, y, hh, a)
            K.append(P.f(Y[6]))
            err = dtype(0)
            for c in range(3):
                s = sum((ecoef[j] * K[j][c] for j in range(7)), dtype(0))
                sc = atol + rtol * np.maximum(np.abs(y[c]), np.abs(Y[6][c]))
                err = max(err, np.max(np.abs(hh * s) / sc))
            steps += 1
            assert np.isfinite(err) and steps < 200000
            if err <= 1:
                hs.append(hh)
                n_acc[to] += 1
                t = t_end if hh == t_end - t else t + hh
                y = Y[6]
            h = hh * (dtype(5) if err == 0 else min(dtype(5), max(dtype(0.2), dtype(0.9) * err ** dtype(-0.2))))
        outs.append(y)
    res = tuple(np.stack([o[c] for o in outs]) for c in (1, 0, 2))
    return res, np.array(hs, dtype), n_acc, steps


def rel_err(got, want):
    """max |got - want| / max |want| over every entry"""
    want = np.asarray(want)
    return float(np.max(np.abs(np.asarray(got, want.dtype) - want)) / np.max(np.abs(want)))


# ------------------------------------------------------------------ the GPU cases (numpy only), shared by the CPU bar and the GPU tests
def _sym_csr(n, u, v, loops=()):
    import scipy.sparse as sp
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    keep = u != v
    u, v = u[keep], v[keep]
    r, c = np.concatenate([u, v, np.asarray(loops, np.int64)]), np.concatenate([v, u, np.asarray(loops, np.int64)])
    M = sp.coo_matrix((np.ones(len(r), np.int8), (r, c)), shape=(n, n)).tocsr()
    M.sum_duplicates()
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32)


def random_graph(n, m, seed, loops=()):
    rng = np.random.default_rng(seed)
    return _sym_csr(n, rng.integers(0, n, m), rng.integers(0, n, m), loops)


def star(n):
    return _sym_csr(n, np.zeros(n - 1, np.int64), np.arange(1, n))


def _inputs(rp, ci, B, seed, beta="rows", w=True, zero_w=False, per_sample=True):
    rng = np.random.default_rng(seed)
    n, nnz = len(rp) - 1, len(ci)
    pI = rng.uniform(0.0, 0.3, (B, n))
    pR = rng.uniform(0.0, 0.1, (B, n))
    init = np.stack([1.0 - pI - pR, pI, pR], axis=-1)
    deg = max(1.0, float(np.diff(rp).mean()))
    row = lambda lo, hi: rng.uniform(lo, hi, (B, n)) if per_sample else np.repeat(rng.uniform(lo, hi, (1, n)), B, axis=0)   # noqa: E731
    bet = row(0.5, 1.5) if beta == "rows" else None
    gam = row(0.1, 0.5)
    wt = rng.uniform(0.2, 1.0, nnz) / deg if w and nnz else None
    if wt is not None and zero_w:
        wt[rng.permutation(nnz)[:nnz // 5]] = 0.0                   # a fifth of the contacts are directed
    if wt is None and bet is not None:
        bet = bet / deg
    return dict(rp=rp, ci=ci, init=init, beta=bet, gamma=gam, w=wt)


def _times(deltaT, maxTime):
    grid = np.arange(0, maxTime, deltaT)
    return np.ascontiguousarray([grid[int(i / deltaT)] for i in range(int(maxTime))], dtype=np.float64)


RTOL, ATOL = 1e-8, 1e-10                # the GPU cases' tolerances: a call takes tens of steps

# The float64 rounding bar of tests/test_gpu_meanfield_grad.py: 64 x the largest |x_f64 - x_longdouble| / max |x_longdouble| over
# the GPU cases' inputs, every gradient array and the outputs, each case replayed on its own dp5_adaptive step list in both
# dtypes.  Measured: 2.65e-15 (tests/test_meanfield_grad_model.py::test_float64_rounding_bar recomputes it and holds it to the
# constant).  64 x leaves room for another summation order and for the step-list difference between the CPU's and the GPU's
# controller; a wrong formula misses the bar by ten orders.
MEASURED_F64_ROUNDING = 2.66e-15
MF_GRAD_RTOL = 64 * MEASURED_F64_ROUNDING


def gpu_cases():
    """name -> dict(rp, ci, init [B, n, 3], beta [B, n] or None, gamma [B, n], w [nnz] or None, t_out); B * n is never a multiple of 256"""
    c = {}
    c["single_node"] = dict(_inputs(np.zeros(2, np.int32), np.zeros(0, np.int32), 1, 1, beta=None), t_out=_times(1, 6))
    c["n257"] = dict(_inputs(*random_graph(257, 700, 2), 1, 3), t_out=_times(1, 6))
    c["n300_B3"] = dict(_inputs(*random_graph(300, 900, 4), 3, 5), t_out=_times(1, 5))
    c["star260"] = dict(_inputs(*star(260), 2, 6), t_out=_times(1, 5))
    c["self_loop"] = dict(_inputs(*random_graph(70, 180, 7, loops=(0, 33)), 2, 8), t_out=_times(1, 6))
    c["directed"] = dict(_inputs(*random_graph(130, 400, 9), 2, 10, zero_w=True), t_out=_times(1, 6))
    c["no_beta_no_w"] = dict(_inputs(*random_graph(90, 200, 11), 2, 12, beta=None, w=False), t_out=_times(1, 6))
    c["deltaT_half"] = dict(_inputs(*random_graph(101, 300, 13), 2, 14), t_out=_times(0.5, 8))
    c["repeated_time"] = dict(_inputs(*random_graph(101, 300, 13), 2, 15), t_out=np.array([0.0, 1.0, 1.0, 2.5, 2.5, 4.0]))
    c["n_out_1"] = dict(_inputs(*random_graph(50, 120, 16), 2, 17), t_out=np.array([0.0]))
    for k, v in c.items():
        assert (v["init"].shape[0] * v["init"].shape[1]) % 256 != 0, k
    return c


def compared_keys(case):
    """the gradients a case is compared on: all four, but without an edge neither w nor beta reaches the outputs.  With
    beta or w None the gradient is the one at 1.  (At n_out = 1 only init's is non-zero; the others are compared to 0.)"""
    return ("init", "beta", "gamma", "w") if len(case["ci"]) else ("init", "gamma")


def grad_out(case, seed=99):
    """a random linear loss: (gI, gS, gR), [n_out, B, n] each"""
    rng = np.random.default_rng(seed)
    B, n = case["gamma"].shape
    return tuple(rng.uniform(-1.0, 1.0, (len(case["t_out"]), B, n)) for _ in range(3))
