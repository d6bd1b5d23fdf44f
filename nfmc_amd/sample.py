"""Public entry points `sample()` / `create_sampler()` with the reference's signature and keyword
plumbing (nfmc/sample.py:20-30, 243-314) for the strategies on this build's path:

    mala, ula, hmc, uhmc, mh, mclmc                       (inner samplers)
    imh / fixed_imh, jump_mala, jump_ula, jump_hmc, jump_uhmc, jump_mh, neutra_hmc, neutra_mh

    adaptive_imh, dlmc (needs `negative_log_likelihood`, like the reference)

Other reference strategies (ess, nuts, jump_ess, tess) are outside the path and raise
ValueError naming what is supported.
"""
from typing import Optional, Tuple, Union

import torch

from .containers import MCMCOutput, NFMCKernel, Sampler
from .flows import Flow
from .potentials import Potential
from .samplers.dlmc import DLMC, DLMCKernel, DLMCParameters
from .samplers.imh import AdaptiveIMH, FixedIMH, IMHKernel, IMHParameters
from .samplers.jump import JumpHMC, JumpMALA, JumpMH, JumpNFMCParameters, JumpUHMC, JumpULA
from .samplers.mcmc import (HMC, MALA, MCLMC, MH, UHMC, ULA, HMCKernel, HMCParameters, LangevinKernel, LangevinParameters,
                            MCLMCKernel, MCLMCParameters, MHKernel, MHParameters)
from .samplers.neutra import NeuTraHMC, NeuTraKernel, NeuTraMH, NeuTraParameters
from .util import create_flow_object, get_supported_samplers


def create_sampler(target: callable,
                   event_shape: Optional[Union[torch.Size, Tuple[int]]] = None,
                   flow: Optional[Union[str, Flow]] = 'realnvp',
                   strategy: str = "imh",
                   negative_log_likelihood: callable = None,
                   kernel_kwargs: Optional[dict] = None,
                   param_kwargs: Optional[dict] = None,
                   inner_kernel_kwargs: Optional[dict] = None,
                   inner_param_kwargs: Optional[dict] = None,
                   device: torch.device = None,
                   flow_kwargs: Optional[dict] = None) -> Sampler:
    """nfmc/sample.py:20-240.  `device` is accepted for signature compatibility; the chain state and the
    flow always live on the current ROCm device."""
    flow_kwargs = flow_kwargs or {}
    kernel_kwargs = kernel_kwargs or {}
    param_kwargs = param_kwargs or {'n_iterations': 100}
    inner_kernel_kwargs = inner_kernel_kwargs or {}
    inner_param_kwargs = dict(inner_param_kwargs or {})

    if flow is not None and not isinstance(flow, str):
        event_shape = flow.event_shape
    elif isinstance(target, Potential):
        event_shape = target.event_shape
    event_shape = tuple(event_shape)
    event_size = int(torch.prod(torch.as_tensor(event_shape)))

    if strategy == "hmc":
        return HMC(event_shape, target, HMCKernel(event_size=event_size, **kernel_kwargs), HMCParameters(**param_kwargs))
    if strategy == "uhmc":
        return UHMC(event_shape, target, HMCKernel(event_size=event_size, **kernel_kwargs), HMCParameters(**param_kwargs))
    if strategy == "mala":
        return MALA(event_shape, target, LangevinKernel(event_size=event_size, **kernel_kwargs),
                    LangevinParameters(**param_kwargs))
    if strategy == "ula":
        return ULA(event_shape, target, LangevinKernel(event_size=event_size, **kernel_kwargs),
                   LangevinParameters(**param_kwargs))
    if strategy == "mh":
        return MH(event_shape, target, MHKernel(event_size=event_size, **kernel_kwargs), MHParameters(**param_kwargs))
    if strategy == "mclmc":
        return MCLMC(event_shape, target, MCLMCKernel(event_size=event_size, **kernel_kwargs), MCLMCParameters(**param_kwargs))

    if strategy == "dlmc" and negative_log_likelihood is None:
        raise ValueError("Unsupported sampling strategy: dlmc without a negative_log_likelihood "
                         "(Negative log likelihood must be provided)")   # sample.py:221-222
    if strategy in ("imh", "fixed_imh", "adaptive_imh", "jump_mala", "jump_ula", "jump_hmc", "jump_uhmc", "jump_mh", "neutra_hmc",
                    "neutra_mh", "dlmc"):
        if flow is None:
            raise ValueError("Flow object must be provided")
        if isinstance(flow, str):
            flow_object = create_flow_object(flow_string=flow, event_shape=event_shape, **flow_kwargs)
            # the reference moves the new flow to its device here (sample.py:118-120 `.to(device)`); this build's
            # equivalent is the packed weight blob the kernels read: uploaded now rather than inside sample()
            bij = getattr(flow_object, 'bijection', None)
            if torch.cuda.is_available() and hasattr(bij, 'packed') and not bij.beyond_kernels():
                bij.packed(torch.device('cuda', torch.cuda.current_device()))
        elif hasattr(flow, 'sample') and hasattr(flow, 'log_prob'):
            flow_object = flow
        else:
            raise ValueError(f"Unknown type for normalizing flow: {type(flow)}")
        if strategy in ("imh", "fixed_imh"):
            return FixedIMH(event_shape, target, IMHKernel(event_shape, flow=flow_object), IMHParameters(**param_kwargs))
        if strategy == "adaptive_imh":
            # sample.py:127-130 builds IMHParameters() and so drops param_kwargs (n_iterations included);
            # deliberate deviation: they are honoured here
            return AdaptiveIMH(event_shape, target, IMHKernel(event_shape, flow=flow_object), IMHParameters(**param_kwargs))
        if strategy in ('jump_mala', 'jump_ula'):
            cls = JumpMALA if strategy == 'jump_mala' else JumpULA
            return cls(event_shape, target, kernel=NFMCKernel(event_shape, flow=flow_object),
                       params=JumpNFMCParameters(**param_kwargs),
                       inner_kernel=LangevinKernel(event_size=event_size, **inner_kernel_kwargs),
                       inner_params=LangevinParameters(**inner_param_kwargs))
        if strategy in ('jump_hmc', 'jump_uhmc'):
            if strategy == 'jump_hmc' and 'n_iterations' not in inner_param_kwargs:
                inner_param_kwargs['n_iterations'] = 5  # sample.py:161-162
            cls = JumpHMC if strategy == 'jump_hmc' else JumpUHMC
            return cls(event_shape, target, kernel=NFMCKernel(event_shape, flow=flow_object),
                       params=JumpNFMCParameters(**param_kwargs),
                       inner_kernel=HMCKernel(event_size=event_size, **inner_kernel_kwargs),
                       inner_params=HMCParameters(**inner_param_kwargs))
        if strategy == 'jump_mh':
            return JumpMH(event_shape, target, kernel=NFMCKernel(event_shape, flow=flow_object),
                          params=JumpNFMCParameters(**param_kwargs),
                          inner_kernel=MHKernel(event_size=event_size, **inner_kernel_kwargs),
                          inner_params=MHParameters(**inner_param_kwargs))
        if strategy == 'dlmc':   # sample.py:220-225
            return DLMC(event_shape, target, negative_log_likelihood, DLMCKernel(event_shape, flow=flow_object),
                        DLMCParameters(**param_kwargs))
        if strategy == 'neutra_mh':
            return NeuTraMH(event_shape, target, MHKernel(event_size=event_size, **inner_kernel_kwargs),
                            MHParameters(**inner_param_kwargs), NeuTraKernel(event_shape, flow=flow_object),
                            NeuTraParameters(**param_kwargs))
        if strategy == 'neutra_hmc':
            return NeuTraHMC(event_shape, target, HMCKernel(event_size=event_size, **inner_kernel_kwargs),
                             HMCParameters(**inner_param_kwargs), NeuTraKernel(event_shape, flow=flow_object),
                             NeuTraParameters(**param_kwargs))
    raise ValueError(f"Unsupported sampling strategy: {strategy} (this build covers {get_supported_samplers()})")


def sample(target: Union[callable, Potential],
           event_shape: Optional[Union[torch.Size, Tuple[int, ...]]] = None,
           flow: Optional[Union[str, Flow]] = 'realnvp',
           strategy: str = "imh",
           n_iterations: int = 100,
           n_warmup_iterations: int = 100,
           n_chains: int = 100,
           x0: torch.Tensor = None,
           warmup: bool = False,
           show_progress: bool = True,
           sampling_time_limit_seconds: Union[float, int] = None,
           warmup_time_limit_seconds: Union[float, int] = None,
           **kwargs) -> MCMCOutput:
    """nfmc/sample.py:243-314.  Keywords beyond the reference's (all optional):
      seed   native Philox stream seed (default: drawn from torch's global generator)
      shard  nfmc_amd.dist.Shard when the chains are split over GPUs
      rng_rounds  10 (default): Philox4x32-10, the library's noise stream.  7: Philox4x32-7 -- an opt-in stream (the fewest
             rounds Random123 reports as passing BigCrush) with 30 % fewer generator instructions, available on the exact-fit
             kernels of mala / hmc / jump_* with a closed-form quadratic target; other launches raise ValueError.
             Warmup (tuning) launches always draw from the 10-round stream, with the device- and the host-side controller alike.
      fuse   'auto' (default): a plain callable `target` that probing reproduces exactly as
             U = sum_j a_j (x_j - b_j)^2 + c (potentials.recognize: an inference from finitely many evaluations,
             logged once) is evaluated in closed form inside the HIP kernels; 'never' / False: always call the Python
             callable (U and grad U by torch autograd on the GPU, the reference's recipe)."""
    if flow == 'None':
        flow = None
    if flow is not None and not isinstance(flow, str):
        event_shape = flow.event_shape
    elif isinstance(target, Potential):
        event_shape = target.event_shape
    elif event_shape is None and hasattr(target, 'event_shape'):
        event_shape = tuple(target.event_shape)   # a `potentials`-package object (sample.py:285-286), duck-typed
    if event_shape is None and x0 is not None:
        event_shape = tuple(x0.shape[1:])   # (the reference fails on `*None` here)
    seed = kwargs.pop('seed', None)
    shard = kwargs.pop('shard', None)
    fuse = kwargs.pop('fuse', 'auto')
    rng_rounds = kwargs.pop('rng_rounds', 10)
    if 'param_kwargs' not in kwargs:
        kwargs['param_kwargs'] = {}
    kwargs['param_kwargs'] = {**kwargs['param_kwargs'],
                              **dict(n_iterations=n_iterations, n_warmup_iterations=n_warmup_iterations)}
    sampler = create_sampler(target=target, event_shape=event_shape, flow=flow, strategy=strategy, **kwargs)
    sampler.seed = seed
    sampler.shard = shard
    sampler.fuse = fuse
    sampler.rng_rounds = rng_rounds
    if x0 is None:
        x0 = torch.randn(size=(n_chains, *event_shape))  # drawn after flow construction, sample.py:304-305
    if warmup:
        warmup_output = sampler.warmup(x0=x0, show_progress=show_progress, time_limit_seconds=warmup_time_limit_seconds)
        if warmup_output.store_samples:       # (not `.samples`: that would copy the whole store to the host)
            flat = warmup_output.samples_device.flatten(0, 1)
            x0 = flat[torch.randperm(len(flat), device=flat.device)][:x0.shape[0]]
        else:
            x0 = warmup_output.running_samples.last_sample
    return sampler.sample(x0=x0, show_progress=show_progress, time_limit_seconds=sampling_time_limit_seconds)
