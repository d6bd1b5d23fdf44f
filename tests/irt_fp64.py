"""fp64 restatement of the item-response-theory target (potentials.ItemResponseTheory), for the host and GPU tests: U, its
gradient and the diagonal of its Hessian written as loops over the students and the questions, the model's log densities
from torch.distributions, start states and exact prior draws.  Nothing here uses the class."""
import torch


class IRTU64:
    """U(x) in fp64, x = (alpha_0 .. alpha_{S-1}, beta_0 .. beta_{Q-1}, mu), l_sq = mu + alpha_s - beta_q:

        U = (mu - m0)^2 / (2 sigma_mu^2) + sum_s alpha_s^2 / (2 sigma_a^2) + sum_q beta_q^2 / (2 sigma_b^2)
            + sum_{(s, q) observed} [log(1 + e^{l_sq}) - y_sq l_sq]

    log(1 + e^l) written as logaddexp(0, l), one loop iteration per student and question.  R (S, Q) of 0 / 1, `observed`
    a bool mask (None: every pair).  Callable on (n, ...) tensors of any dtype; works under autograd."""

    def __init__(self, R, observed=None, mean_ability_prior=(0.75, 1.0), ability_scale=1.0, difficulty_scale=1.0):
        self.R = torch.as_tensor(R).double()
        self.S, self.Q = (int(v) for v in self.R.shape)
        self.M = torch.ones(self.S, self.Q, dtype=torch.bool) if observed is None else torch.as_tensor(observed).bool()
        self.d = self.S + self.Q + 1
        self.m0, self.s_mu = float(mean_ability_prior[0]), float(mean_ability_prior[1])
        self.s_a, self.s_b = float(ability_scale), float(difficulty_scale)

    def _pairs(self):
        return [(s, q) for s in range(self.S) for q in range(self.Q) if bool(self.M[s, q])]

    def prior(self, x):
        x = x.reshape(x.shape[0], -1).double()
        S, Q = self.S, self.Q
        u = (x[:, S + Q] - self.m0) ** 2 / (2 * self.s_mu ** 2)
        for s in range(S):
            u = u + x[:, s] ** 2 / (2 * self.s_a ** 2)
        for q in range(Q):
            u = u + x[:, S + q] ** 2 / (2 * self.s_b ** 2)
        return u

    def __call__(self, x):
        x = x.reshape(x.shape[0], -1).double()
        S, Q = self.S, self.Q
        u = self.prior(x)
        mu = x[:, S + Q]
        for s, q in self._pairs():
            l = mu + x[:, s] - x[:, S + q]
            u = u + torch.logaddexp(torch.zeros_like(l), l) - self.R[s, q] * l
        return u

    def grad(self, x):
        """dU/dx by explicit loops: r_sq = sigmoid(l_sq) - y_sq to alpha_s (+), beta_q (-) and mu (+)."""
        x = x.reshape(x.shape[0], -1).double()
        S, Q = self.S, self.Q
        mu = x[:, S + Q]
        g = torch.zeros_like(x)
        g[:, :S] = x[:, :S] / self.s_a ** 2
        g[:, S:S + Q] = x[:, S:S + Q] / self.s_b ** 2
        g[:, S + Q] = (mu - self.m0) / self.s_mu ** 2
        for s, q in self._pairs():
            r = torch.sigmoid(mu + x[:, s] - x[:, S + q]) - self.R[s, q]
            g[:, s] += r
            g[:, S + q] -= r
            g[:, S + Q] += r
        return g

    def hess_diag(self, x):
        """d^2 U / dx_c^2 by explicit loops: v_sq = p (1 - p), p = sigmoid(l_sq), to alpha_s, beta_q and mu, plus the
        prior precisions."""
        x = x.reshape(x.shape[0], -1).double()
        S, Q = self.S, self.Q
        mu = x[:, S + Q]
        h = torch.zeros_like(x)
        h[:, :S] = 1 / self.s_a ** 2
        h[:, S:S + Q] = 1 / self.s_b ** 2
        h[:, S + Q] = 1 / self.s_mu ** 2
        for s, q in self._pairs():
            p = torch.sigmoid(mu + x[:, s] - x[:, S + q])
            v = p * (1 - p)
            h[:, s] += v
            h[:, S + q] += v
            h[:, S + Q] += v
        return h


class IRTFast64(IRTU64):
    """The same numbers as IRTU64 with the pairs as one (n, S, Q) tensor: the oracle samplers' runs at d = 1023 would take
    minutes through the loops.  Checked against the loops in tests/test_host_irt.py."""

    def _l(self, x):
        S, Q = self.S, self.Q
        return x[:, S + Q, None, None] + x[:, :S, None] - x[:, None, S:S + Q]

    def __call__(self, x):
        x = x.reshape(x.shape[0], -1).double()
        l = self._l(x)
        data = torch.where(self.M, torch.logaddexp(torch.zeros_like(l), l) - self.R * l, torch.zeros_like(l))
        return self.prior(x) + data.sum((1, 2))

    def _scatter(self, x, w, sign_beta):
        S, Q = self.S, self.Q
        out = torch.zeros_like(x)
        out[:, :S] = w.sum(2)
        out[:, S:S + Q] = sign_beta * w.sum(1)
        out[:, S + Q] = w.sum((1, 2))
        return out

    def grad(self, x):
        x = x.reshape(x.shape[0], -1).double()
        S, Q = self.S, self.Q
        r = torch.where(self.M, torch.sigmoid(self._l(x)) - self.R, torch.zeros((), dtype=torch.float64))
        g = self._scatter(x, r, -1.0)
        g[:, :S] += x[:, :S] / self.s_a ** 2
        g[:, S:S + Q] += x[:, S:S + Q] / self.s_b ** 2
        g[:, S + Q] += (x[:, S + Q] - self.m0) / self.s_mu ** 2
        return g

    def hess_diag(self, x):
        x = x.reshape(x.shape[0], -1).double()
        S, Q = self.S, self.Q
        p = torch.sigmoid(self._l(x))
        h = self._scatter(x, torch.where(self.M, p * (1 - p), torch.zeros((), dtype=torch.float64)), 1.0)
        h[:, :S] += 1 / self.s_a ** 2
        h[:, S:S + Q] += 1 / self.s_b ** 2
        h[:, S + Q] += 1 / self.s_mu ** 2
        return h


def model_u64(x, R, observed=None, mean_ability_prior=(0.75, 1.0), ability_scale=1.0, difficulty_scale=1.0):
    """The model's negative log joint from torch.distributions in fp64 -- Normal priors for mu, alpha and beta,
    Bernoulli(logits = l) for the observed answers: U of IRTU64 up to one constant.  Argument validation is off, so a
    non-finite state gives a non-finite U for its own row (as the kernels do) instead of an error for the whole batch."""
    dist = torch.distributions
    x = x.reshape(x.shape[0], -1).double()
    R = torch.as_tensor(R).double()
    S, Q = (int(v) for v in R.shape)
    M = torch.ones(S, Q, dtype=torch.bool) if observed is None else torch.as_tensor(observed).bool()
    alpha, beta, mu = x[:, :S], x[:, S:S + Q], x[:, S + Q]

    def normal(v, mean, scale):
        return dist.Normal(torch.full_like(v, float(mean)), torch.full_like(v, float(scale)), validate_args=False).log_prob(v)
    lp = normal(mu, mean_ability_prior[0], mean_ability_prior[1]) + normal(alpha, 0.0, ability_scale).sum(1)
    lp = lp + normal(beta, 0.0, difficulty_scale).sum(1)
    l = mu[:, None, None] + alpha[:, :, None] - beta[:, None, :]
    ll = dist.Bernoulli(logits=l, validate_args=False).log_prob(R.expand_as(l))
    return -(lp + torch.where(M, ll, torch.zeros_like(ll)).sum((1, 2)))


def start_states(ref, truth, n, seed):
    """n fp64 states (n, d): the generating state plus N(0, 1) / sqrt(hess_diag(truth)) per coordinate -- about one
    posterior standard deviation around it -- rounded through fp32.  `ref` is an IRTU64."""
    g = torch.Generator().manual_seed(seed)
    truth = torch.as_tensor(truth).double().reshape(1, -1)
    sd = 1 / torch.sqrt(ref.hess_diag(truth))
    x = truth + torch.randn(n, truth.shape[1], generator=g, dtype=torch.float64) * sd
    return x.float().double()


def prior_draws(S, Q, n, seed, mean_ability_prior=(0.75, 1.0), ability_scale=1.0, difficulty_scale=1.0):
    """n exact draws (n, S + Q + 1) of the prior, fp64."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, S + Q + 1, generator=g, dtype=torch.float64)
    x[:, :S] *= ability_scale
    x[:, S:S + Q] *= difficulty_scale
    x[:, S + Q] = mean_ability_prior[0] + mean_ability_prior[1] * x[:, S + Q]
    return x
