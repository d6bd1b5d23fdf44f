"""GPU: the interacting-particle target (NFMC_POT_PARTICLES) on the fused HIP kernels against the fp64 CPU oracle, with
the target restated in fp64 as explicit pair sums (tests/particles_fp64.py).

A problem is (P, D, pair): P particles in D dimensions, 'lj' = Lennard-Jones (epsilon = 1, r_min = 1) or 'dw' = the double
well of ParticleSystem.double_well_4 (a = 0, b = -4, c = 0.9, r0 = 4), trap k = 1, temperature 1.  Chains start at
ParticleSystem.start_states(n, seed = d + 1, JITTER): the lattice of spacing r_min (r0) plus N(0, JITTER^2) noise, JITTER =
0.03 r_min or 0.025 r0; _Problem asserts that no pair starts inside 0.8 of the spacing.  The oracle samplers of
oracle/samplers.py run on the same Philox streams with the restatement as target.  The mass diagonals come from H = the median over the starts of the
positive entries of the fp64 diagonal Hessian (of |.| for a coordinate with none: (2, 1) 'dw', whose single pair starts
on the barrier top): MALA inv_mass_diag = sqrt(H), HMC 1 / H, MH STEP 0.5 / sqrt(d H).  Steps are capped as in
tests/test_gpu_varying_effects.py, times a factor (STEP, HMC_STEP): MALA STEP min(0.5, 2.5 d^(-1/3)), HMC
STEP min(0.4, 1.6 d^(-1/4)) with 5 leapfrog steps (2 at d >= 513); ula and uhmc take a tenth (Lennard-Jones) or a quarter
(double well) of those: at a quarter one of the oracle's own unadjusted Lennard-Jones chains at (3, 3) reaches |x| = 97 in
three transitions.

The inputs were chosen on the CPU from the oracle alone, for three conditions: the oracle excludes
under 5 % of the chains as near-ties, its acceptance lies strictly between 0.2 and 0.99, and the restatement's own
fp32-against-fp64 difference of the kept states (the same oracle run in fp32) is under a tenth of the state tolerance.
  * Lennard-Jones gradients are steep and the diagonal Hessian has soft coordinates (H from 0.6 to 245): at the
    varying-effects caps the oracle accepts nothing above 11 particles.  STEP = 1/8 for mala, 1/2 for hmc (1 at D < 3,
    1/4 at 13 and 22 particles: HMC_STEP), 2 for mh.
  * The double well is a four-particle model: on a lattice of spacing r0 the far pairs of a larger system sit high in
    the quartic, U is 2e4 (11 particles) to 2e6 (43) at temperature 1, and fp32 cannot resolve a log ratio of that size
    to MARGIN (the restatement's own fp32 error in U is 4e-3 to 0.4 there).  DW_TEMPERATURE raises the temperature of
    those shapes by a power of 4 so that U is 10 to 150; the kernel then sees beta (a, b, c) scaled by 1/256 .. 1/65536.
  * hmc on the two-particle double well in the plane starts on the barrier top (the pair at r0, curvature -8): five
    leapfrog steps at the cap amplify a rounding error 5e3 times in four transitions, and the restatement in fp32 alone
    uses 0.72 of the state tolerance, above the tenth the third condition allows.  HMC_STEP halves that step (0.005 of
    the tolerance, acceptance 0.98).

Tolerances are the project's (tests/test_gpu_irt.py, quoted in tests/test_gpu_varying_effects.py):
  states        atol 1e-3 + rtol 1e-4
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN = 2e-3 at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.
The oracle ALONE over the whole grid of test 1 (64 chains, 16 at d >= 513, 4 transitions) excludes at most 3.1 % of the
chains (2 of 64); per kind and pair form, largest excluded share and range of acceptance:
  mala  lj 3.1 %, 0.37 .. 0.95    dw 1.6 %, 0.29 .. 0.88
  mh    lj 1.6 %, 0.53 .. 0.74    dw 1.6 %, 0.64 .. 0.92
  hmc   lj 3.1 %, 0.43 .. 0.95    dw 1.6 %, 0.45 .. 0.98
and the restatement's fp32 run stays within 0.065 of the state tolerance (hmc, lj (2, 2); mala and mh under 0.01).
_compare prints the share and _oracle the acceptance of every case.

NeuTra gradient: U~ and its gradient within max(2e-4 of (1 + max |.|), the bound of the existing kinds, 12 x floor), the
floor being the restatement's own fp32-against-fp64 error on the same input in the same normalisation (the rule of
tests/test_gpu_spline_trained.py), computed on the CPU inside the test.  Measured on the CPU: the floor of U~ is 5.6e-6 to
1.1e-3 (largest at lj (43, 3), |U~| up to 1.1e3) and of the gradient 2.6e-7 to 3.4e-6, so 12 x floor is under the existing bound in every case (at most
1.3e-2 against 0.22 for U~, 4.1e-5 against 2e-4 for the gradient) and the existing bound governs.  The flows of tests 3
and 4 are centred on the start lattice (_flow_pair): a flow about the origin puts Lennard-Jones particles on top of each
other.

Shapes (P, D): (2, 1), (2, 2) layout (4, 1); (4, 2) DW4 itself, (4, 2); (3, 3) a particle straddling a quad and a lane and
(5, 3), (4, 4); (11, 3) and (13, 3) = LJ13, (8, 8); (22, 3) (8, 16); (43, 3) (8, 32); (86, 3) (8, 64); (171, 3) and
(341, 3) (16, 64); (16, 2) fills (4, 8) and (8, 1) fills (4, 2) exactly (tests/test_host_particles.py asks the library).
Both pair forms up to d = 129, Lennard-Jones alone above.  64 chains, 16 at d >= 513.

The jump and IMH cases of section 3 also compare the kernel's decisions and log ratios row by row (H.compare_flow_mh,
skip_below_minus_50: overlapping particles give U = inf).  The matrix of section 3b proposes about the start lattice
with 0.3 of the conditional standard deviations there (_flow_centre): the fp64 oracle alone accepts 0.083 to 0.536 of
the proposals up to capacity 128 and 0.052 to 0.401 above, at most 1.0 % of the chains of a case are within MARGIN of a
tie, and some proposals are hopeless (fp64 log ratios down to -588): every case sets skip_below_minus_50.
"""
import copy
import functools
import math

import pytest
import torch

import target_harness as H
from particles_fp64 import Particles64, lattice_sites, min_pair_distance, start_states
from target_harness import Spy as _Spy, imh_run as _imh_run, neutra_grad as _neutra_grad

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4
JITTER = {'lj': 0.03, 'dw': 0.1}
# factors on the varying-effects tests' step caps (mala, hmc) and on MH's proposal scale, chosen on the CPU: see the docstring
STEP = {'mala': {'lj': 0.125, 'dw': 1.0}, 'hmc': {'lj': 0.5, 'dw': 1.0}, 'mh': {'lj': 2.0, 'dw': 1.0}}
UNADJUSTED = {'lj': 0.1, 'dw': 0.25}    # ula and uhmc: this share of the mala and hmc steps
HMC_STEP = {('lj', 2, 1): 1.0, ('lj', 2, 2): 1.0, ('lj', 4, 2): 1.0, ('lj', 8, 1): 1.0, ('lj', 16, 2): 1.0, ('lj', 13, 3): 0.25,
            ('lj', 22, 3): 0.25, ('dw', 2, 2): 0.5}   # else STEP['hmc']
PAIRS = {'lj': 'lennard_jones', 'dw': 'double_well'}
# temperature of the double well above 5 particles (1 elsewhere): see the module docstring
DW_TEMPERATURE = {(11, 3): 256.0, (13, 3): 256.0, (22, 3): 1024.0, (43, 3): 16384.0, (16, 2): 4096.0, (8, 1): 65536.0}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def n_chains(d):
    return 16 if d >= 513 else 64


class _Problem:
    """potential, fp64 restatement (also the oracle's target), starts x0 fp32 (n, d), H (d,) fp64"""

    def __init__(self, P, D, pair, n=None):
        from nfmc_amd.potentials import ParticleSystem
        kw = dict(temperature=DW_TEMPERATURE.get((P, D), 1.0) if pair == 'dw' else 1.0)
        self.pot = ParticleSystem(P, D, PAIRS[pair], **kw)
        self.ref = self.target = Particles64(P, D, PAIRS[pair], **kw)
        self.P, self.D, self.pair, self.d = P, D, pair, P * D
        n = n_chains(self.d) if n is None else n
        x0 = self.pot.start_states(n, self.d + 1, JITTER[pair])
        assert torch.equal(x0, start_states(P, D, self.pot.spacing, n, self.d + 1, JITTER[pair]))
        assert float(min_pair_distance(x0, P, D).min()) > 0.8 * self.pot.spacing
        self.x0 = x0.float()
        h = self.ref.hess_diag(x0)
        pos = torch.where(h > 0, h, torch.full_like(h, float('nan'))).nanmedian(0).values
        self.H = torch.where(torch.isnan(pos), h.abs().median(0).values, pos)
        self.name = '%s P=%d D=%d d=%d' % (pair, P, D, self.d)

    def imd(self, kind):
        if kind in ('mala', 'ula'):
            return torch.sqrt(self.H)
        if kind in ('hmc', 'uhmc'):
            return 1 / self.H
        return STEP['mh'][self.pair] * 0.5 / torch.sqrt(self.d * self.H)

    def step(self, kind):
        f = UNADJUSTED[self.pair] if kind in ('ula', 'uhmc') else 1.0
        if kind in ('mala', 'ula'):
            return f * STEP['mala'][self.pair] * min(0.5, 2.5 * self.d ** (-1 / 3))
        if kind in ('hmc', 'uhmc'):
            f *= HMC_STEP.get((self.pair, self.P, self.D), STEP['hmc'][self.pair])
            return f * min(0.4, 1.6 * self.d ** (-1 / 4))
        return 0.0

    def leapfrog(self):
        return 2 if self.d >= 513 else 5


@functools.lru_cache(maxsize=None)
def _problem(P, D, pair, n=None):
    return _Problem(P, D, pair, n)


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)


def _sampler(kind, p, T, L=None, target=None, h=None, imd=None):
    """every kind with the problem's mass diagonal of that kind"""
    return H.mcmc_sampler(kind, p.d, p.pot if target is None else target, T, p.step(kind) if h is None else h,
                          p.leapfrog() if L is None else L, p.imd(kind) if imd is None else imd, imd_kinds=H.KINDS)


def _oracle(kind, p, T, noise, L=None):
    return H.oracle_trace(kind, p.x0, p.target, T, p.step(kind), noise, p.leapfrog() if L is None else L,
                          p.imd(kind).float().double(), imd_kinds=H.KINDS, label='%s %s' % (kind, p.name))


SMALL = [(2, 1), (2, 2), (4, 2), (3, 3), (5, 3), (11, 3), (13, 3), (22, 3), (43, 3), (16, 2), (8, 1)]
LARGE = [(86, 3), (171, 3), (341, 3)]
GRID = [(P, D, pair) for P, D in SMALL for pair in ('lj', 'dw')] + [(P, D, 'lj') for P, D in LARGE]
IDS = ['%s-%dx%d' % (pair, P, D) for P, D, pair in GRID]


def _run_against_oracle(monkeypatch, kind, P, D, pair, T):
    """the native stream, states alone: the kernel's masks and log ratios are not recorded for this kind"""
    p = _problem(P, D, pair)
    H.native_matches_oracle(monkeypatch, p, kind, T, _sampler(kind, p, T), lambda noise: _oracle(kind, p, T, noise),
                            seed=777 + p.d, what='%s %s' % (kind, p.name), compare=_compare, decisions=None)


# ------------------------------------------------------------------------- 1. mala, mh, hmc against the fp64 oracle
@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
@pytest.mark.parametrize('P,D,pair', GRID, ids=IDS)
def test_mcmc_matches_oracle(dev, monkeypatch, kind, P, D, pair):
    _run_against_oracle(monkeypatch, kind, P, D, pair, 4)


# ------------------------------------------------------------------------- 2. ula and uhmc at reduced steps
@pytest.mark.parametrize('kind', ['ula', 'uhmc'])
@pytest.mark.parametrize('P,D,pair', [(2, 2, 'dw'), (4, 2, 'dw'), (3, 3, 'lj'), (13, 3, 'lj'), (43, 3, 'dw'), (171, 3, 'lj')])
def test_unadjusted_matches_oracle(dev, monkeypatch, kind, P, D, pair):
    _run_against_oracle(monkeypatch, kind, P, D, pair, 3)


SIGMA = {'lj': 0.05, 'dw': 0.15}


def _flow_pair(p, seed=5, n_hidden=None, spline=False):
    """A perturbed flow (oracle.flow.perturb_, every parameter touched) whose data-side elementwise layer is then centred
    on the start lattice with scale SIGMA: x = f^-1(z) is the lattice plus SIGMA times a distorted normal, so proposals
    and NeuTra states are configurations of finite energy.  A flow about the origin puts the particles of a
    Lennard-Jones system on top of each other: U ~ 1e11, and every comparison would be between overflows."""
    from nfmc_amd.flows import Flow, RealNVP
    from nfmc_amd.util import create_flow_object
    from oracle import flow as oflow
    d = p.d
    ck = {} if n_hidden is None else {'conditioner_kwargs': {'n_hidden': n_hidden}}
    if spline:
        of = oflow.perturb_(oflow.Flow(oflow.CRQNSF((d,))), seed, 0.3)
        f = create_flow_object('c-rqnsf', (d,))
    else:
        of = oflow.perturb_(oflow.Flow(oflow.RealNVP((d,), **ck)), seed, 0.2)
        f = Flow(RealNVP((d,), **ck))
    sites = lattice_sites(p.P, p.D, p.pot.spacing).reshape(-1).float()
    with torch.no_grad():
        first = of.bijection.layers[0]                        # z' = e^{log_scale} x + shift
        first.log_scale.add_(-math.log(SIGMA[p.pair]))
        first.shift.add_(-sites / SIGMA[p.pair])
    f.load_state_dict(of.state_dict())
    return f, of.double()


def _latents(p, seed):
    return torch.randn(p.x0.shape[0], p.d, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _flow_starts(p, of, seed):
    """fp32 draws of the flow itself: chains that start where the proposals land accept a fair share of them (from the
    low-energy lattice starts the oracle accepts almost none, and the comparison would be of rejections alone)"""
    with torch.no_grad():
        return of.bijection.inverse(_latents(p, seed))[0].float()


D8_9_39 = [(4, 2, 'dw'), (3, 3, 'lj'), (13, 3, 'lj')]


# ------------------------------------------------------------------------- 3. a jump tail and the flow-MH register kernels
def _jump_oracle(x0, target, flow, T, Kin, h, imd, seed):
    """oracle.samplers.jump_sample spelled out so that the uniforms of the inner transitions are kept beside those of the
    jumps (jump_sample keeps the jumps' alone): a Trace with one log ratio and one log u per transition, for _compare."""
    from oracle import samplers as osamp
    noise = osamp.PhiloxNoise(seed, dtype=torch.float64)
    tr, x = osamp.Trace(), x0
    for i in range(T):
        base = i * (Kin + 1)
        inner = osamp.mcmc_sample(x, target, 'langevin', Kin, h, imd, adjustment=True, noise=noise, step0=base)
        js = osamp.jump_transition(inner.last, target, flow, base + Kin, noise, True, (x0.shape[1],))
        tr.samples += inner.samples + [js.x.clone()]
        tr.log_ratios += inner.log_ratios + [js.log_alpha]
        tr.uniforms += inner.uniforms + [js.log_u]
        tr.n_accepted_jumps += int(js.mask.sum())
        x = js.x
    return tr


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('P,D,pair', D8_9_39)
def test_jump_mala_matches_oracle(dev, monkeypatch, fuse_tail, P, D, pair):
    """Three outer iterations of one mala transition and a jump: six transitions, three of them jumps, every one under
    the tie-aware rule of _compare (the jump's log ratio and log u like the inner ones').  With fuse_tail the jump runs
    behind the mala launch; at d = 39 ParticleSystem.jump_tail_ok declines that route because it measures slower, so
    the test overrides it there: the tail kernels of the eight-coordinate layouts exist for C callers and are checked
    like the others."""
    from nfmc_amd.containers import NFMCKernel
    from nfmc_amd.samplers import jump, mcmc
    from oracle import samplers as osamp
    n, T, Kin, seed = 64, 3, 1, 31337
    p = _problem(P, D, pair)
    d, h, imd = p.d, p.step('mala'), p.imd('mala').float()
    f, of = _flow_pair(p)
    rec = H.FlowRecord(monkeypatch)                           # the jumps' decisions and log ratios, tail or flow-MH kernel
    split, flow_mh = [], []
    orig, orig_fm = jump.split_flow_mh, jump.launch_flow_mh
    monkeypatch.setattr(jump, 'split_flow_mh', lambda *a, **k: split.append(1) or orig(*a, **k))
    monkeypatch.setattr(jump, 'launch_flow_mh', lambda *a, **k: flow_mh.append(1) or orig_fm(*a, **k))
    spy = _Spy(monkeypatch)
    s = jump.JumpMALA((d,), p.pot, NFMCKernel((d,), flow=f), jump.JumpNFMCParameters(n_iterations=T),
                      mcmc.LangevinKernel(event_size=d, step_size=h, inv_mass_diag=imd),
                      mcmc.LangevinParameters(n_iterations=Kin))
    s.seed, s.fuse_jump_tail = seed, fuse_tail
    assert p.pot.jump_tail_ok() == (d <= 32)
    monkeypatch.setattr(type(p.pot), 'jump_tail_ok', lambda self: True)
    xs = _flow_starts(p, of, 17)
    out = s.sample(xs, show_progress=False)
    assert not spy.calls and not split                        # inner loop and jump fused
    assert len(flow_mh) == (0 if fuse_tail else T)            # each jump in the tail, or on the flow-MH kernel
    tr = _jump_oracle(xs.double(), p.target, of, T, Kin, h, imd.double(), seed)
    ref = osamp.jump_sample(xs.double(), p.target, of, 'langevin', T, Kin, h, inv_mass_diag=imd.double(),
                            noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    assert torch.equal(tr.stacked(), ref.stacked()) and tr.n_accepted_jumps == ref.n_accepted_jumps
    got, what = out.samples.reshape(T * (Kin + 1), n, d), 'jump_mala %s tail=%s' % (p.name, fuse_tail)
    assert (rec.tails, rec.launches) == ((T, 0) if fuse_tail else (0, T))
    got_m, got_lr = rec.stacked()
    H.compare_flow_mh(got_m, got_lr, ref.flow_steps, what, c=H.affine_c(d), margin=MARGIN, skip_below_minus_50=True, min_share=0.9,
                      comparable=H.jump_comparable(got, ref.stacked().float(), Kin, ATOL, RTOL))
    keep = _compare(got, tr, what)
    assert out.statistics.n_attempted_jumps == n * T
    assert out.statistics.n_accepted_jumps == int(got_m.sum())
    assert abs(out.statistics.n_accepted_jumps - tr.n_accepted_jumps) <= T * int((~keep).sum())   # the excluded chains' jumps


@pytest.mark.parametrize('spline', [False, True])
@pytest.mark.parametrize('P,D,pair', D8_9_39)
def test_imh_runs_on_the_register_flow_mh_kernel(dev, monkeypatch, P, D, pair, spline):
    """Affine and spline ('c-rqnsf') instantiations of the register flow-MH kernel for kind 11.  A perturbed flow's
    proposals put Lennard-Jones particles close together: most are rejected, some with U = inf, and the oracle and the
    kernel must agree on every chain that is no near-tie."""
    from oracle import samplers as osamp
    n, T = 64, 4
    p = _problem(P, D, pair)
    d, seed = p.d, 4711 + p.d
    f, of = _flow_pair(p, 3 if spline else 9, spline=spline)
    xs = _flow_starts(p, of, 23)
    rec = H.FlowRecord(monkeypatch)
    out = _imh_run(monkeypatch, p.pot, d, f, xs, T, seed)
    tr = osamp.imh_sample(xs.double(), p.target, of, T, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    what = '%s imh %s' % ('c-rqnsf' if spline else 'realnvp', p.name)
    got_m, got_lr = rec.stacked()
    c = H.spline_c(d, of, tr.flow_steps)[0] if spline else H.affine_c(d)
    # proposals with U = inf or a log ratio below -50 must be rejected; the others' log ratios are compared
    H.compare_flow_mh(got_m, got_lr, tr.flow_steps, what, c=c, margin=MARGIN, skip_below_minus_50=True, min_share=0.9,
                      u_sensitivity=H.u_sensitivity_of(tr.flow_steps, p.target))     # Lennard-Jones: U(x') is steep in x'
    _compare(out.samples.reshape(T, n, d), tr, what)
    assert out.statistics.n_accepted_trajectories == int(got_m.sum())

# ------------------------------------------------------------------------- 3b. the flow-MH matrix
# capacity -> (P, D, pair), d = P D ragged in it.  jump_tail_ok stays as the class has it: from d = 33 the jumps of the
# jump cases run on the flow-MH kernel, not behind the inner launch
FLOW_SHAPES = {4: (3, 1, 'dw'), 8: (2, 3, 'lj'), 16: (4, 3, 'dw'), 32: (8, 3, 'lj'), 64: (16, 3, 'lj'), 128: (33, 3, 'lj'),
               256: (66, 3, 'lj'), 512: (100, 3, 'lj')}
FLOW_SKIP_CAPS = (4, 8, 16, 32, 64, 128, 256, 512)    # some proposals are hopeless at every capacity: see the docstring
FLOW_CASES = H.flow_cases({cap: P * D for cap, (P, D, _pair) in FLOW_SHAPES.items()})
FLOW_TESTS = ('test_flow_mh_matrix',)
# the 120 KB LDS bound: two affine coupling layers of width 8 at the ragged capacity 512 are 132 KB by themselves
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8'}
FLOW_SHRINK = 0.3


def _flow_centre(p):
    """Proposals about the start lattice (the mean of the file's starts), FLOW_SHRINK of the conditional standard deviations there:
    configurations of finite energy, as _flow_pair's"""
    return H.local_fit(p, FLOW_SHRINK, at='starts')


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh).  The inner steps of the jump cases shrink with the
    proposal (FLOW_SHRINK^2 for MALA, a tenth of FLOW_SHRINK for HMC, whose mass diagonal is the lattice's and not the
    proposal's), so that a chain is still inside it when the jump comes."""
    P, D, pair = FLOW_SHAPES[case.cap]
    p = _problem(P, D, pair, 96)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL, h_mala=FLOW_SHRINK ** 2 * p.step('mala'),
                    h_hmc=0.1 * FLOW_SHRINK * p.step('hmc'), imd=lambda kind: p.imd(kind).float(),
                    refused=H.flow_case_id(case) in FLOW_REFUSED, centre=_flow_centre(p), skip_caps=FLOW_SKIP_CAPS)


# ------------------------------------------------------------------------- 4. NeuTra gradient and trajectory (VALU kernels)
def neutra_reference(of, ref, z, d):
    """(U~, grad U~) in fp64 and the restatement's own fp32 error in each: (u64, g64, floor_u, floor_g), the floors in the
    normalisation of the check -- U~ absolute, the gradient per row relative to 1 + the row's largest entry."""
    from oracle import samplers as osamp
    out = []
    for flow, target, dt in ((of, ref, torch.float64), (copy.deepcopy(of).float(), ref.u32, torch.float32)):
        zz = z.to(dt).detach().clone().requires_grad_(True)
        u = osamp.neutra_adjusted_target(flow, target, (d,))(zz)
        g, = torch.autograd.grad(u.sum(), zz)
        out.append((u.detach().double(), g.double()))
    (u64, g64), (u32, g32) = out
    floor_u = float((u32 - u64).abs().max())
    floor_g = float(((g32 - g64).abs().amax(dim=1) / (1 + g64.abs().amax(dim=1))).max())
    return u64, g64, floor_u, floor_g


D9_39_129 = [(3, 3, 'lj', 8), (3, 3, 'dw', 4), (13, 3, 'lj', 16), (13, 3, 'dw', 32), (43, 3, 'lj', 16), (43, 3, 'dw', 8)]


@pytest.mark.parametrize('P,D,pair,nh', D9_39_129)
def test_neutra_gradient_matches_fp64_autograd(dev, P, D, pair, nh):
    """U~(z) = U(f^-1(z)) - log|det J_{f^-1}(z)| and its gradient from the VALU NeuTra kernel against fp64 autograd
    through oracle/flow.py and the pair sums, at standard normal latents z (f^-1(z) is a distorted lattice: _flow_pair)."""
    from nfmc_amd import hip
    p = _problem(P, D, pair)
    d = p.d
    f, of = _flow_pair(p, 3, n_hidden=nh)
    z = _latents(p, 100 + d).float()
    u_ref, g_ref, floor_u, floor_g = neutra_reference(of, p.ref, z.double(), d)
    rc, u, g = _neutra_grad(dev, f, p.pot, z)
    assert rc == hip.OK
    fin = torch.isfinite(u_ref) & torch.isfinite(g_ref).all(1)
    assert float(fin.float().mean()) > 0.9
    bound_u = max(2e-4 * (1 + float(u_ref[fin].abs().max())), 12 * floor_u)
    bound_g = max(2e-4, 12 * floor_g)
    err_u = float((u.double() - u_ref)[fin].abs().max())
    err_g = float(((g.double() - g_ref).abs().amax(dim=1) / (1 + g_ref.abs().amax(dim=1)))[fin].max())
    print('%s H=%d: U~ error %.2e (floor %.2e, bound %.2e), gradient error %.2e (floor %.2e, bound %.2e)'
          % (p.name, nh, err_u, floor_u, bound_u, err_g, floor_g, bound_g))
    assert err_u <= bound_u and err_g <= bound_g


@pytest.mark.parametrize('P,D,pair,nh', [(3, 3, 'lj', 8), (13, 3, 'lj', 16), (43, 3, 'dw', 16)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, P, D, pair, nh):
    p = _problem(P, D, pair)
    h = 0.2 / (SIGMA[pair] * math.sqrt(float(p.H.max())))      # a latent step: the flow scales it by SIGMA
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, _flow_pair(p, 9, n_hidden=nh), T=1, L=4, h=h, seed=12, atol=1e-3,
                                      share=0.93, accept_slack=4)


# ------------------------------------------------------------------------- 5. device warmup against the fp64 controller
@pytest.mark.parametrize('kind,every', [('mala', 1), ('hmc', 2)])
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, every):
    """LJ13 (d = 39).  As tests/test_gpu_warmup.py does for the other kinds."""
    n = 70
    p = _problem(13, 3, 'lj', n)
    d, lm = p.d, float(p.H.max())
    h0 = 0.3 * (0.5 * d ** (-1 / 4) / math.sqrt(lm) if kind == 'hmc' else 0.5 * d ** (-1 / 3) / lm)
    H.warmup_matches_controller(monkeypatch, p, kind, W=8, T=4, L=4, every=every, h0=h0, imd0=torch.ones(d), seed=4242 + d,
                                what='particles %s %s n=%d every=%d' % (kind, p.name, n, every), ties=0.05)


# ------------------------------------------------------------------------- 6. coincident Lennard-Jones particles
@pytest.mark.parametrize('P,D', [(4, 2), (8, 3), (8, 1)])
def test_a_proposal_with_coincident_particles_is_rejected_and_counted(dev, P, D):
    """Random-walk MH on replayed noise with a unit mass diagonal, from the exact lattice (jitter 0: every coordinate a
    multiple of 0.5, so x + (y - x) = y exactly in fp32).  Transition 0 moves particle 1 onto particle 0 in every chain:
    s = 0, U(x') = inf, the log ratio is not finite: rejected and counted.  Transition 1 proposes x' = x (zero noise,
    log ratio 0 against log u < 0): accepted, so the count is that of transition 0 alone and the kernel went on."""
    p = _problem(P, D, 'lj')
    d, n, T = p.d, 64, 2
    x0 = p.pot.start_states(n, 1, 0.0).float()
    assert torch.equal(x0.double() * 2, (x0.double() * 2).round())
    normals = torch.zeros(T, n, d)
    normals[0, :, D:2 * D] = x0[:, :D] - x0[:, D:2 * D]
    s = _sampler('mh', p, T, imd=torch.ones(d, dtype=torch.float64))
    s.replay = (normals, torch.full((T, n), 0.5))
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.equal(out.samples.reshape(T, n, d), x0.expand(T, n, d))
    assert st.n_nonfinite_log_ratios == n and st.n_accepted_trajectories == n


@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_coincident_starts_are_rejected_and_counted(dev, kind):
    """Chains that START with particle 1 on particle 0: U(x) = inf and a NaN force, every log ratio is non-finite.  The
    adjusted kernels reject every proposal and count it (n_nonfinite_log_ratios), as for the existing kinds' overflows;
    the states stay where they are, finite."""
    p = _problem(13, 3, 'lj')
    d, n, T = p.d, 64, 3
    x0 = p.x0.clone()
    x0[:, 3:6] = x0[:, 0:3]
    s = _sampler(kind, p, T, L=3, h=0.01, imd=torch.ones(d, dtype=torch.float64))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.isfinite(out.samples).all()
    assert torch.equal(out.samples.reshape(T, n, d)[-1], x0)
    assert st.n_accepted_trajectories == 0 and st.n_nonfinite_log_ratios == n * T


# ------------------------------------------------------------------------- 7. determinism, 9. kept states of sample()
@pytest.mark.parametrize('kind,P,D,pair', [('mala', 13, 3, 'lj'), ('hmc', 4, 2, 'dw'), ('hmc', 43, 3, 'lj')])
def test_two_runs_are_bitwise_equal_and_kept_states_are_the_dense_runs(dev, kind, P, D, pair):
    """Every unordered pair is summed twice in a fixed order, with no atomics: two identical runs give the same bits.
    thinning / max_samples keep states of the dense run, in order."""
    p = _problem(P, D, pair)
    d, n, T = p.d, p.x0.shape[0], 5
    runs = []
    for _ in range(2):
        s = _sampler(kind, p, T)
        s.seed = 7
        runs.append(s.sample(p.x0, show_progress=False))
    assert torch.equal(runs[0].samples, runs[1].samples)
    assert runs[0].statistics.n_accepted_trajectories == runs[1].statistics.n_accepted_trajectories > 0
    dense = runs[0].samples.reshape(T, n, d)
    s = _sampler(kind, p, T)
    s.seed = 7
    s.params.thinning, s.params.max_samples = 2, 2
    kept = s.sample(p.x0, show_progress=False).samples.reshape(-1, n, d)
    assert kept.shape[0] == 2
    idx = [next(t for t in range(T) if torch.equal(kept[i], dense[t])) for i in range(2)]
    assert idx == sorted(idx) and len(set(idx)) == 2


def test_sample_keeps_the_states_of_the_dense_run(dev):
    """The public entry: sample(ParticleSystem.double_well_4(), strategy='mala') with thinning against the same call
    without, from start_states."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import ParticleSystem
    pot = ParticleSystem.double_well_4()
    n, T = 64, 6
    x0 = pot.start_states(n, 3, JITTER['dw']).float()
    kw = dict(flow=None, strategy='mala', n_iterations=T, n_chains=n, show_progress=False, seed=11, x0=x0,
              kernel_kwargs={'step_size': 0.05})
    dense = sample(pot, **kw).samples.reshape(T, n, 8)
    kept = sample(pot, param_kwargs={'thinning': 3}, **kw).samples.reshape(-1, n, 8)
    assert torch.isfinite(dense).all() and not torch.equal(dense[0], dense[-1])
    assert torch.equal(kept, dense[[0, 3]])


# ------------------------------------------------------------------------- 8. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    p = _problem(13, 3, 'lj')
    pot = p.pot
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_PARTICLES == 11 and pd.n_components == 13 and not pd.b
    assert pd.a % 16 == 0 and pot.descriptor(dev).a == pd.a                           # cached per device
    H.refusing_entry_points(dev, pot, p.x0, functools.partial(_flow_pair, p))


def test_the_fit_step_refuses_kind_11(dev):
    p = _problem(4, 2, 'dw')
    H.fit_step_refuses(dev, p.pot, p.x0, _flow_pair(p)[0])


def test_philox7_and_bad_descriptors_are_refused(dev):
    """check_particles' codes: a NULL a, P < 2 and a P that does not give d = P D with D in 1 .. 3 are EINVAL; a misaligned
    a is EALIGN."""
    from nfmc_amd import hip
    p = _problem(4, 3, 'lj')
    assert p.d == 12
    bad = [('a', 0, hip.EINVAL), ('n_components', 0, hip.EINVAL), ('n_components', 1, hip.EINVAL), ('n_components', -4, hip.EINVAL),
           ('n_components', 5, hip.EINVAL),                                               # 12 % 5 != 0
           ('n_components', 3, hip.EINVAL), ('n_components', 2, hip.EINVAL),                  # D = 4, D = 6
           ('n_components', 24, hip.EINVAL), ('n_components', 2 ** 30, hip.EINVAL), ('a', 'misaligned', hip.EALIGN)]
    H.bad_descriptors_are_refused(dev, p.pot, p.x0, _flow_pair(p)[0], bad,
                                  ok=[('n_components', 6), ('n_components', 12)])            # the same d as D = 2 and D = 1: well formed


def test_limits_are_unchanged(dev):
    H.limits_are_unchanged()
