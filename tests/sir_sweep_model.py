"""The CPU model of the Monte-Carlo candidate sweep (`gnode_sir_mc_philox_sweep`, `outbreak_sizes_mc`) and its cases, stated
once (a helper, not a test).  numpy only.

The model: for each candidate c, `sir_schedule_model.sir_events_schedule` from the start p whose row c is replaced -- (0, 1, 0)
for "seed", (0, 0, 1) for "immunise"; an id outside [0, n) replaces nothing -- under the phase row taken from the candidate's
shift on (step t reads phase[shift + t]; the coins are those of step t).  sums[c] = `sir_model.curves` summed over the
trajectories; ever[c, s] = the nodes of trajectory s that left S and did not start in R (t_rec = 0 marks an R start and nothing
else: a recovery takes a step).

The cases are the shapes of tests/schedule_cases.py with a phase row three entries longer than T, four to six candidates each
(`candidates`) and sims = the shape's own sims // C, so that C * sims trajectories are at most what the shape's own test runs.
tests/test_sir_sweep_host.py runs `live` on every (case, action, shifts) the GPU module uses."""
import functools
from types import SimpleNamespace

import numpy as np

import schedule_cases as K
import sir_cases as SC
import sir_model as M
from sir_schedule_model import schedule_thresholds, sir_events_schedule

ROW = {"seed": (0.0, 1.0, 0.0), "immunise": (0.0, 0.0, 1.0)}
EXTRA = 3                                                           # entries of the phase row beyond T


def sweep(n, rp, ci, p, cands, shifts, action, W, G, phase, sims, T, rng_seed, sim_offset=0, thresholds=None):
    """(sums uint64 [C, T, 3], ever uint32 [C, sims]) of the model; thresholds: `schedule_thresholds` of W and G, if at hand."""
    THR, TG = thresholds or schedule_thresholds(W, G, len(ci), n)
    phase = np.asarray(phase)
    sums, ever = np.zeros((len(cands), T, 3), dtype=np.uint64), np.zeros((len(cands), sims), dtype=np.uint32)
    done = {}
    for j, (c, k) in enumerate(zip(cands, shifts)):
        c, k = int(c), int(k)
        if (c, k) not in done:
            q = np.array(p, dtype=np.float64)
            if 0 <= c < n:
                q[c] = ROW[action]
            assert k >= 0 and k + T <= len(phase)
            t_inf, t_rec = sir_events_schedule(n, rp, ci, q, THR, TG, phase[k:], sims, T, rng_seed, sim_offset)
            done[(c, k)] = (M.curves(t_inf, t_rec, T).sum(0, dtype=np.uint64), ((t_inf >= 0) & (t_rec != 0)).sum(1).astype(np.uint32))
        sums[j], ever[j] = done[(c, k)]
    return sums, ever


def infections(sums):
    """int64 [C]: `gnode.dmp.infections` on the integer sums"""
    s = sums.astype(np.int64)
    return s[:, -1, 1] + s[:, -1, 2] - s[:, 0, 2]


# ----------------------------------------------------------------------------------------------------------------- cases
KEYS = ["er-small/init", "hubs/init", "global-lists/init", "large/init", "everybody"]


def candidates(n, rp, p):
    """-1 (no change), a node the start already infects, the hub, the last node, the hub again, and a node of degree 0 where
    there is one."""
    deg = np.diff(rp)
    hub = int(np.argmax(deg))
    out = [-1, int(np.flatnonzero(p[:, 1] == 1.0)[0]), hub, n - 1, hub]
    lone = np.flatnonzero(deg == 0)
    return out + [int(lone[0])] if lone.size else out


@functools.lru_cache(maxsize=None)
def case(key):
    """A schedule_cases case as the sweep takes it: the start as p [n, 3], the phase row EXTRA entries longer than T (the
    phases in rotation, so the last entry differs from the one before it), the candidates, the mixed shifts (the hub at 0 and
    at EXTRA: the last entry of the row is read), and sims per candidate."""
    c = K.case(key)
    p = np.asarray(c.start, dtype=np.float64) if np.ndim(c.start) == 2 else M.one_hot_init(c.n, c.start)
    P = len(c.W)
    phase = np.concatenate([c.phase, [(int(c.phase[-1]) + 1 + i) % P for i in range(EXTRA)]]).astype(np.int32)
    cands = candidates(c.n, c.rp, p)
    mixed = [0, 1, 0, 2, EXTRA, 1][:len(cands)]
    return SimpleNamespace(key=key, base=c, n=c.n, rp=c.rp, ci=c.ci, p=SC._frozen(p), W=c.W, G=c.G, P=P, phase=SC._frozen(phase), T=c.T,
                           L=len(phase), cands=cands, mixed=mixed, zeros=[0] * len(cands), sims=c.sims // len(cands), rng_seed=c.rng_seed)


# what the GPU module runs: every case under ("seed", mixed shifts) and ("immunise", no shifts), er-small under all four
RUNS = [(k, a, s) for k in KEYS for a, s in (("seed", "mixed"), ("immunise", "zeros"))] + [("er-small/init", "seed", "zeros"),
                                                                                            ("er-small/init", "immunise", "mixed")]


@functools.lru_cache(maxsize=None)
def _thresholds(key):
    c = case(key)
    return schedule_thresholds(c.W, c.G, len(c.ci), c.n)


@functools.lru_cache(maxsize=None)
def expected(key, action, shifts, sims=None, sim_offset=0):
    """(sums, ever) of the model for a case, read-only; shifts is "mixed" or "zeros"."""
    c = case(key)
    out = sweep(c.n, c.rp, c.ci, c.p, c.cands, getattr(c, shifts), action, c.W, c.G, c.phase, c.sims if sims is None else sims, c.T,
                c.rng_seed, sim_offset, thresholds=_thresholds(key))
    return tuple(SC._frozen(a) for a in out)


def live(key, action, shifts):
    """On the model's own output: some candidate changes the sums against -1; "immunise" lowers and "seed" raises the number
    ever infected for some candidate (`everybody`, where w = 1 infects all n whatever the start, must instead reach n for every
    seeded candidate and change a row of the sums); under mixed shifts the hub shifted differs from the hub unshifted; and the
    identity between ever and the sums holds."""
    c = case(key)
    sums, ever = expected(key, action, shifts)
    assert c.cands[0] == -1 and c.cands[2] == c.cands[4] and 4 <= len(c.cands) <= 6 and c.sims >= 4
    assert len(c.cands) * c.sims <= c.base.sims
    assert any(not np.array_equal(sums[j], sums[0]) for j in range(1, len(c.cands))), f"{key}: no candidate changes the sums"
    size = infections(sums)
    assert np.array_equal(ever.sum(1, dtype=np.int64), size)
    print(f"{key} {action} {shifts}: ever infected per candidate {size.tolist()} of {c.sims} x {c.n}")
    sh = getattr(c, shifts)
    others = size[[j for j in range(1, len(sh)) if sh[j] == sh[0]]]     # the candidates under the calendar of -1 (the hub among them)
    if action == "immunise":
        assert (others < size[0]).any(), f"{key}: immunising lowers nothing"
    elif key == "everybody":
        assert (size == c.sims * c.n).all()
    else:
        assert (others > size[0]).any(), f"{key}: seeding raises nothing"
    if shifts == "mixed":
        assert c.mixed[2] == 0 and c.mixed[4] == EXTRA and c.phase[-1] != c.phase[-2]
        assert not np.array_equal(sums[2], sums[4]), f"{key}: the shift changes nothing"


# ------------------------------------------------------------------------------------------------------------------ tree
# DMP is exact on a tree: the comparison of tests/test_gpu_sir_sweep.py, every node a candidate, shifts 0 / 1 / 2 in rotation
TREE_T, TREE_SIMS, TREE_RNG, TREE_ACTION = 10, 2000, 4321, "seed"


def tree_shifts(cands):
    return [int(c) % 3 for c in cands]


def tree_dmp(cands):
    """float64 [C]: `infections` of the DMP model's sizes (tests/dmp_sweep_schedule_model.py) for the tree comparison"""
    import dmp_sweep_schedule_model as D
    n, rp, ci, W, G, p = K.tree()
    sz = D.sizes(rp, ci, W, G, K.TREE_PHASE, p, list(cands), tree_shifts(cands), TREE_ACTION, None, TREE_T)
    return sz[:, -1, 1] + sz[:, -1, 2] - sz[:, 0, 2]


def tree_ever(cands, sims=TREE_SIMS, rng_seed=TREE_RNG):
    """uint32 [C, sims] of the model for the tree comparison"""
    n, rp, ci, W, G, p = K.tree()
    return sweep(n, rp, ci, p, list(cands), tree_shifts(cands), TREE_ACTION, W, G, K.TREE_PHASE, sims, TREE_T, rng_seed)[1]


def tree_ratio(dmp, ever):
    """float64 [C]: |dmp - mean(ever[c])| / (5 std(ever[c]) / sqrt(sims) + 1 / sims): inside the bound iff <= 1"""
    ever = np.asarray(ever, dtype=np.float64)
    sims = ever.shape[1]
    return np.abs(np.asarray(dmp) - ever.mean(1)) / (5.0 * ever.std(1) / np.sqrt(sims) + 1.0 / sims)
