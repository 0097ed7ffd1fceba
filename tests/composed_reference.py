"""A whole-series reference for the filter families the CPU oracle does not restate: the guided filters (LG1D AFFINE / OPTIMAL,
UCSV OPTIMAL) and the marginal UCSV family.  No step arithmetic is written down here.  One filter step is composed from pieces
that are pinned on their own:

  1. ancestors      the oracle's resampler at the filter's time index (orc_filter_draw_ancestors: weights_resample /
                    weights_resample_systematic, pinned by the bootstrap parity tests)
  2. normals        particle i takes element i & 1 of the pair i >> 1 at (stream, t, slot SLOT_NORMAL0 + k) (orc_state_normals)
  3. the step       the library's host twin applied to ALL rows of the ancestor's state (smc_host_guided_steps /
                    smc_host_rb_steps, pinned against extended precision by tests/test_guided_host.py and tests/test_rbpf_host.py)
  4. normalisation  the oracle's segmented fixed-point normalize (orc_filter_put_step: weights_normalize)

The step at t = 0 of a guided filter is the bootstrap first step (smc_spec.h, comment at model_guided): the oracle's own
bootstrap_filter; of the marginal family it is the twin with first = True on the normals of t = 0.  What this pins is the order
of gather, normals and time index, the rows loaded, and the weights; the step arithmetic itself is the host tests' business.
"""
import numpy as np

NONE, AFFINE, OPTIMAL = 0, 1, 2
LG, UC, RB = 1, 3, 4
ROWS = {LG: 1, UC: 3, RB: 4}
NORMALS = {LG: 1, UC: 3, RB: 2}


class ComposedFilter:
    """one filter: init(y0), step(y); the traces lm / es, logZ as the running sum in step order, snapshot()"""

    def __init__(self, L, ob, model, raw, n, seg=0, seed=1, stream=0, kind=NONE, par=None, systematic=False):
        assert (model == RB and kind == NONE) or (model in (LG, UC) and kind in (AFFINE, OPTIMAL))
        self.L, self.ob, self.model, self.kind = L, ob, model, kind
        self.d, self.nz, self.n = ROWS[model], NORMALS[model], int(n)
        self.seed, self.stream, self.systematic = int(seed), int(stream), bool(systematic)
        self.f = ob.ExternalFilter(self.d, self.n, seg, self.seed, self.stream, systematic)
        self.seg, self.nseg = self.f.seg, self.f.nseg
        self.set_params(raw, par)
        self.t, self.x, self.logZ, self.lm, self.es = 0, None, 0.0, [], []

    def set_params(self, raw, par=None):
        self.raw = np.array(raw, dtype=np.float64)
        self.par = None if par is None else np.array(par, dtype=np.float64)
        assert (self.kind == AFFINE) == (self.par is not None)

    def set_rng(self, seed, stream):
        """a reseed or a new stream id in the middle of a series: the time index goes on"""
        self.seed, self.stream = int(seed), int(stream)
        self.f.set_rng(self.seed, self.stream)

    # the three choices a kernel can get wrong; separate so that a test can break one on purpose
    def _normals(self, k):
        return self.ob.state_normals(self.seed, self.stream, self.t, self.ob.SLOT_NORMAL0 + k, self.n)

    def _gather(self, a):
        return self.x[:, a]

    def _twin(self, xp, z, y, first=False):
        if self.model == RB:
            return self.L.host_rb_steps(self.raw, xp, z, y, first)
        return self.L.host_guided_steps(self.model, self.raw, self.kind, self.par, xp, z, y)

    def _put(self, x, logw):
        lm, ess = self.f.put_step(x, logw)
        self.x = x
        self.logZ = lm if self.t == 0 else self.logZ + lm
        self.t += 1
        self.lm.append(lm)
        self.es.append(ess)
        return lm, ess

    def init(self, y0):
        assert self.t == 0
        if self.model == RB:
            z = np.stack([self._normals(k) for k in range(self.nz)])
            x, logw = self._twin(np.zeros((self.d, self.n)), z, y0, first=True)
        else:
            b = self.ob.Filter(self.model, self.raw, self.n, seg=self.seg, seed=self.seed, stream=self.stream)
            b.bootstrap_filter(y0)
            x, _, _, logw = b.state()
        return self._put(x, logw)

    def step(self, y):
        a = self.f.draw_ancestors()
        xp = np.ascontiguousarray(self._gather(a))
        z = np.stack([self._normals(k) for k in range(self.nz)])
        x, logw = self._twin(xp, z, y)
        return self._put(x, logw)

    def snapshot(self):
        """(x [d][n], w [n], ancestors [n], C, m, S, S2hi, S2lo): the per-filter slices of test_gpu_guided.snapshot"""
        x, w, a, _ = self.f.state()
        return (x, w, a) + tuple(self.f.weights_raw())


def stack(snaps):
    """snapshots of the filters of a handle in the handle's layouts: x [d][n_theta][n], everything else [n_theta][...]"""
    return tuple(np.stack([s[k] for s in snaps], axis=1 if k == 0 else 0) for k in range(len(snaps[0])))


def run_series(L, ob, model, raws, n, seg, seed, y, kind=NONE, pars=None, systematic=False, streams=None, cls=ComposedFilter):
    """a batched handle's series: parameter row (and proposal row) per filter, stream = the filter's index unless streams says
    otherwise -> dict(lm [T][n_theta], es [T][n_theta], logZ [n_theta], snap = stacked snapshot, first = the same after t = 0)"""
    raws = np.atleast_2d(np.asarray(raws, dtype=np.float64))
    nth = len(raws)
    lm, es, logZ, snaps, firsts = np.zeros((len(y), nth)), np.zeros((len(y), nth)), np.zeros(nth), [], []
    for th in range(nth):
        f = cls(L, ob, model, raws[th], n, seg=seg, seed=seed, stream=th if streams is None else int(streams[th]), kind=kind,
                par=None if pars is None else np.atleast_2d(pars)[th], systematic=systematic)
        f.init(y[0])
        firsts.append(f.snapshot())
        for t in range(1, len(y)):
            f.step(y[t])
        lm[:, th], es[:, th], logZ[th] = f.lm, f.es, f.logZ
        snaps.append(f.snapshot())
    return dict(lm=lm, es=es, logZ=logZ, snap=stack(snaps), first=stack(firsts), seg=f.seg, nseg=f.nseg)


def first_mismatch(dev, ref, names=("x", "w", "ancestors", "C", "m", "S", "S2hi", "S2lo")):
    """the name of the first quantity of two snapshots that is not the same bits (values for the integer ones), or None"""
    for name, u, v in zip(names, dev, ref):
        u, v = np.asarray(u), np.asarray(v)
        if u.shape != v.shape:
            return name + " (shape)"
        if u.dtype == np.float64:
            u, v = (np.ascontiguousarray(q, dtype=np.float64).view(np.uint64) for q in (u, v))
        if not np.array_equal(u, v):
            return name
    return None
