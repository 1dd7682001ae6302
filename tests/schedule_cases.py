"""The cases of the rate-schedule tests, stated once (a helper, not a test): the tree comparison's inputs, the three-phase
schedules on the shapes of tests/sir_cases.py with their expected events from tests/sir_schedule_model.py, and the liveness
checks on those.  numpy only; tests/test_schedule_model.py runs every liveness check without a GPU, the GPU modules reach the
same cached arrays."""
import functools
from types import SimpleNamespace

import numpy as np

import sir_cases as SC
import sir_model as M
from sir_init_model import tree_init
from sir_schedule_model import schedule_thresholds, sir_events_schedule

# ------------------------------------------------------------------------------------------------------------- the tree
TREE_T, TREE_SIMS, TREE_RNG = 12, 20_000, 1234
TREE_PHASE = np.asarray([0, 0, 0, 0, 1, 1, 1, 2, 2, 0, 0, 1], dtype=np.int32)      # entry 0 is never read; phases revisited


@functools.lru_cache(maxsize=None)
def tree():
    """(n, rowptr, col, W, G, p): open, a quarter of the contacts, closed but for the certain entries; gamma, 2.5 gamma, gamma."""
    n, rp, ci, w, gamma = SC.tree_case()
    W = [w, 0.25 * w, (w == 1.0).astype(np.float64)]
    G = [gamma, np.minimum(2.5 * gamma, 1.0), gamma]
    return n, rp, ci, [SC._frozen(a) for a in W], [SC._frozen(a) for a in G], SC._frozen(tree_init())


@functools.lru_cache(maxsize=None)
def tree_events():
    n, rp, ci, W, G, p = tree()
    THR, TG = schedule_thresholds(W, G, len(ci), n)
    return tuple(SC._frozen(a) for a in sir_events_schedule(n, rp, ci, p, THR, TG, TREE_PHASE, TREE_SIMS, TREE_T, TREE_RNG))


# ------------------------------------------------------------------------------------------------------------ the shapes
# phase by step, by T: open (the drawn weights), closed (w = 0), other weights and gamma, phase 0 revisited, a change at T - 1
SHAPE_PHASE = {15: [0, 0, 0, 0, 1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 2], 12: [0, 0, 0, 1, 1, 2, 2, 0, 0, 0, 0, 2],
               10: [0, 0, 0, 1, 2, 2, 0, 0, 0, 2], 8: [0, 0, 0, 1, 2, 2, 0, 2]}
SHAPE_RNG = {"er-small": 21, "hubs": 22, "global-lists": 23, "large": 24}
KINDS = ["er-small", "hubs", "global-lists", "large"]


def shape_tables(kind, n, nnz, seeds):
    """(W, G) of the three phases of a shape: `sir_cases.edge_weights`, the closed phase, and a second draw of both."""
    w, gamma = SC.edge_weights(kind, n, nnz, seeds)
    rng = np.random.default_rng(SC.EDGE_RATE_SEED[kind] + 1000)
    w2, gamma2 = rng.uniform(0.05, 0.9, nnz), rng.uniform(0.05, 0.6, n)
    epos = rng.permutation(nnz)
    w2[epos[:nnz // 10]], w2[epos[nnz // 10:nnz // 10 + nnz // 20]] = 0.0, 1.0
    gamma2[rng.permutation(n)[:n // 20]] = 1.0
    return [w, np.zeros(nnz), w2], [gamma, gamma, gamma2]


def _shape(kind, start, sims=None, sim_offset=0):
    _, n, m, seeds, shape_sims, T = SC.LARGE if kind == "large" else SC.SHAPE[kind]
    rp, ci = SC.csr(kind, n, m)
    W, G = shape_tables(kind, n, len(ci), seeds)
    st = seeds if start == "seeds" else SC.mixed_start(kind, n, rp)
    fields = dict(kind=f"{kind}/{start}", shape=(kind, n, m), n=n, rp=rp, ci=ci, start=st, W=W, G=G,
                  phase=np.asarray(SHAPE_PHASE[T], dtype=np.int32), sims=sims or shape_sims, T=T, rng_seed=SHAPE_RNG[kind],
                  sim_offset=sim_offset, closed=1)
    return SimpleNamespace(**{k: SC._frozen(v) if isinstance(v, np.ndarray) else v for k, v in fields.items()})


def _everybody():
    """`er300_component` with w = 1: everybody is infected within the eccentricity, then only recovery coins are drawn; gamma
    0 up to the switch, 1 from it: everybody infected before the switch recovers exactly at the switch step."""
    n, rp, ci, seed = SC.er300_component()
    ecc = int(SC.bfs_depth(rp, ci, seed, n).max())
    T = ecc + 5
    phase = np.asarray([0] + [0] * (ecc + 1) + [1] * (T - ecc - 2), dtype=np.int32)
    return SimpleNamespace(kind="everybody", shape=None, n=n, rp=rp, ci=ci, start=[seed], W=[np.ones(len(ci))] * 2, G=[0.0, 1.0],
                           phase=phase, sims=32, T=T, rng_seed=4, sim_offset=0, closed=None, switch=ecc + 2)


CASES = {
    **{f"{k}/init": functools.partial(_shape, k, "init") for k in KINDS},
    "er-small/seeds": functools.partial(_shape, "er-small", "seeds"),
    "everybody": _everybody,
}


@functools.lru_cache(maxsize=None)
def case(key):
    return CASES[key]()


class Expected:
    """The model's output for a case, read-only: events, and counts (under the row-0 rule of the start) and curves on demand."""

    def __init__(self, c, sims=None, sim_offset=None):
        THR, TG = schedule_thresholds(c.W, c.G, len(c.ci), c.n)
        self.t_inf, self.t_rec = sir_events_schedule(c.n, c.rp, c.ci, c.start, THR, TG, c.phase, c.sims if sims is None else sims, c.T,
                                                     c.rng_seed, c.sim_offset if sim_offset is None else sim_offset)
        self.t_inf.setflags(write=False)
        self.t_rec.setflags(write=False)
        self._T, self._seeded = c.T, np.ndim(c.start) == 1

    @functools.cached_property
    def counts(self):
        return SC._frozen(M.counts(self.t_inf, self.t_rec, self._T, hold_row0=self._seeded))

    @functools.cached_property
    def curves(self):
        return SC._frozen(M.curves(self.t_inf, self.t_rec, self._T))


@functools.lru_cache(maxsize=None)
def expected(key):
    return Expected(case(key))


# ------------------------------------------------------------------------------------------------------ liveness checks
def live_schedule(c, want):
    """On the model's own output: (1) a quarter of the connected (node, trajectory) pairs left S -- of those that started
    susceptible, where the start is drawn; (2) every open phase sees an infection and a recovery; (3) in the closed phase some
    entry has an infected source next to a susceptible target in a pre-step state, and no node is infected."""
    t_inf, t_rec = want.t_inf.astype(np.int32), want.t_rec.astype(np.int32)
    connected = np.diff(c.rp) > 0
    if np.ndim(c.start) == 2:
        left = float((t_inf > 0)[:, connected].sum()) / float((t_inf != 0)[:, connected].sum())
    else:
        left = float((t_inf >= 0)[:, connected].sum()) / (t_inf.shape[0] * int(connected.sum()))
    print(f"{c.kind}: {left:.3f} of the (connected node, trajectory) pairs left S")
    assert left >= 0.25
    steps = np.arange(c.T)
    for p in range(len(c.W)):
        mine = steps[1:][c.phase[1:] == p]
        assert mine.size, f"{c.kind}: phase {p} governs no step"
        if p == c.closed:
            continue
        assert np.isin(t_inf, mine).any(), f"{c.kind}: no infection in phase {p}"
        assert np.isin(t_rec, mine).any(), f"{c.kind}: no recovery in phase {p}"
    src = np.repeat(np.arange(c.n), np.diff(c.rp))
    tried = False
    for t in steps[1:][c.phase[1:] == c.closed]:
        assert not (t_inf == t).any(), f"{c.kind}: an infection in the closed step {t}"
        inf_before = (t_inf >= 0) & (t_inf < t) & ~((t_rec >= 0) & (t_rec < t))
        sus_before = (t_inf < 0) | (t_inf >= t)
        tried = tried or bool((inf_before[:, src] & sus_before[:, c.ci]).any())
    assert tried, f"{c.kind}: no entry was tried in the closed phase"
    assert c.phase[c.T - 1] != c.phase[c.T - 2], f"{c.kind}: no change at step T - 1"
