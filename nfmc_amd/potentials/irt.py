"""The one-parameter item-response-theory model (csrc/pot_irt.hpp)."""
import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _finite_fp32, _pair, _positive_fp32


class ItemResponseTheory(Potential):
    """The one-parameter item-response-theory model (the Inference Gym's `SyntheticItemResponseTheory`): a hierarchical
    posterior with crossed random effects.  S students answer Q questions; `responses` (S, Q) holds 1 for a correct and 0
    for a wrong answer (numbers or bools, NaN = missing), `observed` is an optional (S, Q) bool mask, and a pair is used
    when it is observed and not NaN:

        mu ~ N(m0, sigma_mu^2),  alpha_s ~ N(0, sigma_a^2),  beta_q ~ N(0, sigma_b^2),
        y_sq ~ Bernoulli(sigmoid(l_sq)),  l_sq = mu + alpha_s - beta_q

    with (m0, sigma_mu) = `mean_ability_prior`, sigma_a = `ability_scale`, sigma_b = `difficulty_scale`; the defaults are
    the Inference Gym's.  Sampled on d = S + Q + 1 coordinates x = [alpha (S) | beta (Q) | mu] (`unpack` / `pack`
    convert).  With precisions p = 1 / sigma^2 and r_sq = sigmoid(l_sq) - y_sq over the used pairs, constants dropped:

        U = 1/2 p_mu (mu - m0)^2 + 1/2 p_a sum_s alpha_s^2 + 1/2 p_b sum_q beta_q^2 + sum_sq [softplus(l_sq) - y_sq l_sq]
        dU/dalpha_s = p_a alpha_s + sum_q r_sq,  dU/dbeta_q = p_b beta_q - sum_s r_sq,  dU/dmu = p_mu (mu - m0) + sum r_sq

    Validated in fp64 on the host: responses 2-D with S, Q >= 1 and 0 or 1 wherever used; the three scales > 0 and
    finite in fp32, their precisions too; m0 finite in fp32.  `synthetic` draws a data set from the model.  The fused
    kernels evaluate it in the mcmc, flow-MH and NeuTra launch families (NeuTra on its VALU kernels, conditioners of at
    most 32 units) for d up to 1024, with no cap on S Q; every other family runs on the split or composed path
    (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False
    fused_families = VALU_FAMILIES

    def __init__(self, responses, observed=None, mean_ability_prior=(0.75, 1.0), ability_scale=1.0, difficulty_scale=1.0):
        R = torch.as_tensor(responses)
        if R.dim() != 2 or R.shape[0] < 1 or R.shape[1] < 1:
            raise ValueError('responses must be 2-D (S, Q) with S, Q >= 1, got shape %s' % (tuple(R.shape),))
        R = R.detach().to('cpu', torch.float64)
        used = ~torch.isnan(R)
        if observed is not None:
            ob = torch.as_tensor(observed).detach().to('cpu')
            if ob.dtype != torch.bool or ob.shape != R.shape:
                raise ValueError('observed must be a bool mask of shape %s, got %s of shape %s'
                                 % (tuple(R.shape), ob.dtype, tuple(ob.shape)))
            used = used & ob
        if not bool(((R == 0) | (R == 1) | ~used).all()):
            raise ValueError('responses must be 0 or 1 wherever they are observed')
        m0, sigma_mu = _pair(mean_ability_prior, 'mean_ability_prior', '(mean, scale)', sized=True)
        self.mean_ability_mean = _finite_fp32('mean_ability_prior mean', m0)
        self.mean_ability_scale = _positive_fp32('mean_ability_prior scale', sigma_mu)
        self.ability_scale = _positive_fp32('ability_scale', ability_scale)
        self.difficulty_scale = _positive_fp32('difficulty_scale', difficulty_scale)
        # the kernels read the precisions, so they too must be positive and finite in fp32
        self.p_mu = _positive_fp32('1 / mean_ability_prior scale^2', self.mean_ability_scale ** -2)
        self.p_a = _positive_fp32('1 / ability_scale^2', self.ability_scale ** -2)
        self.p_b = _positive_fp32('1 / difficulty_scale^2', self.difficulty_scale ** -2)
        self.n_students, self.n_questions = (int(v) for v in R.shape)
        self.event_shape = (self.n_students + self.n_questions + 1,)
        self.observed = used.contiguous()
        self.responses = torch.where(used, R, torch.zeros_like(R)).contiguous()   # fp64 master, 0 where unused
        self._dev = {}

    @classmethod
    def synthetic(cls, n_students, n_questions, seed, missing=0.25, **prior):
        """(potential, truth): (mu, alpha, beta) drawn from the prior given by `prior` (the constructor's keywords), the
        responses from the model, every pair dropped with probability `missing`; all draws in fp64 from one CPU
        torch.Generator seeded with `seed`.  `truth` is the packed generating state (d,), fp64."""
        S, Q = int(n_students), int(n_questions)
        if S < 1 or Q < 1 or not 0.0 <= float(missing) <= 1.0:
            raise ValueError('n_students, n_questions >= 1 and 0 <= missing <= 1, got %r, %r, %r' % (n_students, n_questions, missing))
        proto = cls(torch.zeros(1, 1), **prior)   # validates the prior
        g = torch.Generator().manual_seed(int(seed))
        mu = proto.mean_ability_mean + proto.mean_ability_scale * torch.randn((), generator=g, dtype=torch.float64)
        alpha = proto.ability_scale * torch.randn(S, generator=g, dtype=torch.float64)
        beta = proto.difficulty_scale * torch.randn(Q, generator=g, dtype=torch.float64)
        prob = torch.sigmoid(mu + alpha[:, None] - beta[None, :])
        R = (torch.rand(S, Q, generator=g, dtype=torch.float64) < prob).to(torch.float64)
        observed = torch.rand(S, Q, generator=g, dtype=torch.float64) >= float(missing)
        pot = cls(R, observed, **prior)
        return pot, pot.pack(mu, alpha, beta)

    def _copy(self, device, dtype=torch.float32):
        """(responses, mask) of `device` in `dtype`, made once per (device, dtype)."""
        return self._cached((str(device), dtype), lambda: (self.responses.to(device, dtype).contiguous(),
                                                           self.observed.to(device, dtype).contiguous()))

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        R, M = self._copy(xf.device, xf.dtype)
        S, Q = self.n_students, self.n_questions
        alpha, beta, mu = xf[:, :S], xf[:, S:S + Q], xf[:, S + Q]
        l = mu[:, None, None] + alpha[:, :, None] - beta[:, None, :]               # (n, S, Q)
        # softplus(l) as logaddexp(0, l): exact in every range (torch's softplus is the identity above l = 20), and its
        # derivative is sigmoid(l) everywhere
        data = torch.sum(M * (torch.logaddexp(l.new_zeros(()), l) - R * l), dim=(1, 2))
        dm = mu - self.mean_ability_mean
        return (data + (0.5 * self.p_mu) * dm * dm + (0.5 * self.p_a) * torch.sum(alpha * alpha, dim=1)
                + (0.5 * self.p_b) * torch.sum(beta * beta, dim=1))

    def unpack(self, x):
        """(mean_ability (...), ability (..., S), difficulty (..., Q)) of states x (..., S + Q + 1)."""
        x = self._event_states(x)
        S, Q = self.n_students, self.n_questions
        return x[..., S + Q], x[..., :S], x[..., S:S + Q]

    def pack(self, mean_ability, ability, difficulty):
        """The state x (..., S + Q + 1) of (mean_ability (...), ability (..., S), difficulty (..., Q)); the leading
        shapes broadcast.  Inverse of `unpack`."""
        ability = torch.as_tensor(ability)
        dt = ability.dtype if ability.is_floating_point() else torch.get_default_dtype()
        mu, a, b = (torch.as_tensor(v, dtype=dt, device=ability.device) for v in (mean_ability, ability, difficulty))
        S, Q = self.n_students, self.n_questions
        if a.dim() < 1 or a.shape[-1] != S or b.dim() < 1 or b.shape[-1] != Q:
            raise ValueError('ability must end in S = %d and difficulty in Q = %d entries, got shapes %s, %s'
                             % (S, Q, tuple(a.shape), tuple(b.shape)))
        lead = torch.broadcast_shapes(mu.shape, a.shape[:-1], b.shape[:-1])
        return torch.cat([a.expand(lead + (S,)), b.expand(lead + (Q,)), mu.expand(lead)[..., None]], dim=-1)

    def data_block(self):
        """The kernels' view of the responses (NFMC_POT_ITEM_RESPONSE, include/nfmc_hip.h): (Q, SA) fp32 on the CPU,
        SA = 4 ceil(S / 4), entry [q, s] = the response of student s to question q where it is used and -1 where it is
        not and in the padding s >= S."""
        S, Q = self.n_students, self.n_questions
        A = torch.full((Q, 4 * ((S + 3) // 4)), -1.0, dtype=torch.float32)
        A[:, :S] = torch.where(self.observed, self.responses, torch.full_like(self.responses, -1.0)).t().float()
        return A

    def descriptor(self, device):
        def make():
            par = torch.tensor([self.mean_ability_mean, self.p_mu, self.p_a, self.p_b], dtype=torch.float64)
            return self.data_block().to(device).contiguous(), par.to(device, torch.float32).contiguous()
        A, par = self._cached((str(device), 'descriptor'), make)
        return hip.NfmcPotential(hip.POT_ITEM_RESPONSE, self.n_students, hip.ptr(A), hip.ptr(par), 0.0, 0.0)
