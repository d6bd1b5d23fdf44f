"""fp64 numpy restatement of the running diagnostics' stream algebra, written from the formulas there:
an accumulator that sees the kept draws block by block and never holds more than 2 L rows of them, and the additive
sums in the layout of nfmc_chain_diagnostics_f32 that follow from it.  It shares no code with the library and none with
diagnostics_fp64.py, which is the yardstick it is held against."""
import numpy as np


class Stream:
    """State for n chains of d coordinates, L lags, K_planned draws: shift s, shifted sum S, half-chain sums, the first L
    and the last L shifted draws (the last ones in a ring indexed by draw number), lag products P_l summed over chains."""

    def __init__(self, n, d, max_lag, n_planned, dtype=np.float64):
        self.n, self.d, self.L, self.Kp = int(n), int(d), int(max_lag), int(n_planned)
        self.dtype = dtype                      # the precision the shifted draws are rounded to for products and rows
        self.K = 0
        self.s = np.zeros((n, d))
        self.S = np.zeros((n, d))
        self.half = np.zeros((4, n, d))         # sum, sum of squares of the first half; the same of the second
        self.head = np.zeros((self.L, n, d))
        self.tail = np.zeros((self.L, n, d))    # draw t in row t mod L
        self.P = np.zeros((self.L + 1, d))

    def update(self, block, first_draw):
        block = np.asarray(block, dtype=np.float64)
        if first_draw != self.K:
            raise ValueError('block starts at draw %d, %d seen' % (first_draw, self.K))
        h = self.Kp // 2
        for x in block:
            t = self.K
            if t == 0:
                self.s = x.copy()
            y = x - self.s
            yr = y.astype(self.dtype).astype(np.float64)
            self.S += y
            if t < h:
                self.half[0] += y
                self.half[1] += y * y
            if t >= self.Kp - h:
                self.half[2] += y
                self.half[3] += y * y
            self.P[0] += (yr * yr).sum(axis=0)
            for l in range(1, min(self.L, t) + 1):
                self.P[l] += (yr * self.tail[(t - l) % self.L]).sum(axis=0)
            if t < self.L:
                self.head[t] = yr
            if self.L:
                self.tail[t % self.L] = yr
            self.K += 1

    def sums(self, group=1):
        K, n, d, L = self.K, self.n, self.d, self.L
        mu = self.S / K
        m = mu + self.s
        acov = np.zeros((L + 1, d))
        head_l = np.zeros((n, d))
        tail_l = np.zeros((n, d))
        for l in range(min(L, K - 1) + 1):
            if l > 0:
                head_l = head_l + self.head[l - 1]
                tail_l = tail_l + self.tail[(K - l) % L]
            per_chain = -mu * (2 * self.S - head_l - tail_l) + (K - l) * mu * mu
            acov[l] = (self.P[l] + per_chain.sum(axis=0)) / K
        out = {'sum_m': m.sum(axis=0), 'sum_m2': (m * m).sum(axis=0), 'acov': acov}
        if K == self.Kp:
            h = K // 2
            mh = np.stack([self.s + self.half[0] / h, self.s + self.half[2] / h])
            s2h = np.stack([(self.half[1] - self.half[0] ** 2 / h) / (h - 1), (self.half[3] - self.half[2] ** 2 / h) / (h - 1)])
            out.update(sum_mh=mh.sum(axis=(0, 1)), sum_mh2=(mh * mh).sum(axis=(0, 1)), sum_s2h=s2h.sum(axis=(0, 1)))
        else:   # the half-chains were those of the plan, not of what was seen
            out.update({k: np.full(d, np.nan) for k in ('sum_mh', 'sum_mh2', 'sum_s2h')})
        mg = m.reshape(n // group, group, d)
        mk = mg.mean(axis=1)
        bt = mg.var(axis=1, ddof=1) if group > 1 else np.zeros_like(mk)
        out.update(sum_mu=mk.sum(axis=0), sum_mu2=(mk * mk).sum(axis=0), sum_bt=bt.sum(axis=0))
        return out


def feed(x, blocks, max_lag, n_planned=None, group=1, dtype=np.float64):
    """The sums after feeding the draws of x (K, n, d) in blocks of the given sizes (which must add up to at most K)."""
    K, n, d = x.shape
    st = Stream(n, d, max_lag, K if n_planned is None else n_planned, dtype)
    t = 0
    for b in blocks:
        st.update(x[t:t + b], t)
        t += b
    return st.sums(group)
