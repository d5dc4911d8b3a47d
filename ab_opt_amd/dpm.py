"""FullDPM: the diffusion driver over the HIP denoiser (host-side loop, device-side everything else).

Mirrors AbDock/src/modules/diffusion/dpm_full.py:115-367 (`FullDPM`) and
AbDesign/diffab/modules/diffusion/dpm_full.py:105-319 (no prmsd head / obj).  Differences that are
deliberate and MI355X-first:
  * the loop never leaves the device: states live in a preallocated (T+1)-slot trajectory and are
    copied to the host once, after the last step (the reference does a D2H of every state per step,
    dpm_full.py:300);
  * noise comes from a counter-based Philox stream inside the transition kernel, or is injected
    (`noise=`) to replay a recorded reference run;
  * the loop can be captured ONCE into a hipGraph and replayed (`graph=True`, or automatically from the second call with the same
    shapes and options): every per-step scalar is a kernel argument baked into its node, the Philox stream position is read from a
    16-byte device buffer at execution time, inputs are copied into the graph's static buffers before a replay.
"""
import collections
import ctypes
import dataclasses
import math
import weakref
import os
import torch
import torch.nn as nn

from . import hip
from .modules import (EpsilonNet, RotationTransition, PositionTransition, AminoacidCategoricalTransition, pRMSDCa, _Derived, _range_guarded)


@dataclasses.dataclass(frozen=True)
class _LoopSpec:
    """One denoising loop, from step t_start down to 0 (or for stop_after steps).  Everything below FullDPM._run takes the loop as this one value, and a
    captured loop's cache key holds it whole: an option added here tells graphs apart with no further edit."""
    t_start: int
    stop_after: int | None = None
    sample_structure: bool = True
    sample_sequence: bool = True
    ppl_masked: bool = True                     # perplexity over the generated residues (sample) or over all of them (optimize)
    optimize_mode: bool = False                 # the net's third output is the position update's noise whatever `obj` is
    use_bias_cache: bool | None = None          # None: FullDPM._denoise decides by free memory, once
    constrained: bool = False                   # the loop's inputs end with aa_allowed, the allowed residue types per residue (the contents are data, not key)
    timesteps: tuple | int = 0                  # the steps the loop visits: 0 every step t_start .. 1; K > 0 the K evenly respaced ones, respaced_steps(t_start, K);
                                                # a tuple: these (t_start first, strictly decreasing, >= 1)
    query_row_tiles: int = 0                    # 16-row tiles the generated rows of the loop's longest sample fill (FullDPM._denoise settles it from the masks, once
                                                # per call); 0: the loop holds no row list (include/abopt.h: abopt_eps_net_step, query_row_tiles)
    seq_temperature: float = 1.0                # tau: the temperature of the predicted residue-type distribution of every step (include/abopt.h: seq_temperature)
    noise_scale: float = 1.0                    # lambda: the scale of the structure noise of every step; both 1: the steps carry tempered = 0
    guided: bool = False                        # every step is followed by hip.guide_positions and the loop's inputs end with `role` (behind aa_allowed; the contents
                                                # are data, not key); False: the launches of a loop without the six fields below, which then keep their defaults
    guide_attract: float = 0.0                  # w_att, r_att, w_rep, r_rep, max_shift of include/abopt.h: abopt_guide_positions
    guide_attract_radius: float = 0.0
    guide_repel: float = 0.0
    guide_repel_radius: float = 0.0
    guide_max_shift: float = 0.0
    guide_decay: int = 0                        # k of the step weight g(u) = (u / num_steps)^k on w_att and w_rep, for the step that lands on u


def respaced_steps(t_start, steps=None, timesteps=None):
    """The steps a loop from t_start down to 0 visits (0, where it lands, is implied), as a strictly decreasing tuple that starts at t_start.
    steps = K, 1 <= K <= t_start: the K steps tau_K .. tau_1 of the evenly respaced sub-sequence tau_i = (i t_start + K // 2) // K (tau_0 = 0, tau_K = t_start; the
    strided sampling of improved DDPM).  timesteps: the list itself, checked.  Neither: every step, t_start .. 1.  Both: an error."""
    T = int(t_start)
    if steps is not None and timesteps is not None:
        raise ValueError('give steps= or timesteps=, not both')
    if timesteps is not None:
        ts = tuple(int(t) for t in timesteps)
        if not ts or ts[0] != T or ts[-1] < 1 or any(a <= b for a, b in zip(ts, ts[1:])):
            raise ValueError(f'timesteps must start at step {T}, decrease strictly and end at 1 or above (0 is implied), got {ts[:4]}{"..." if len(ts) > 4 else ""}')
        return ts
    if steps is None:
        return tuple(range(T, 0, -1))
    K = int(steps)
    if not 1 <= K <= T:
        raise ValueError(f'steps must be between 1 and {T}, got {steps}')
    return tuple((i * T + K // 2) // K for i in range(K, 0, -1))


def _spec_timesteps(t_start, steps, timesteps):
    """_LoopSpec.timesteps of sample(steps=, timesteps=) / optimize(...), in its one spelling: 0 where every step is visited, so that such a call IS the plain loop
    (same graph key too), K for the evenly respaced K steps however they were asked for, the tuple for any other list."""
    ts = respaced_steps(t_start, steps, timesteps)
    if len(ts) == int(t_start):
        return 0
    return len(ts) if ts == respaced_steps(t_start, len(ts)) else ts


def _graph_key(spec, inputs, token):
    """A captured loop serves calls with this device, these shapes, this spec and these packed weights (`token`: whoever stores the key keeps it alive)."""
    res_feat, pair_feat, _, mask_res = inputs[:4]
    return (res_feat.device.index, *mask_res.shape, tuple(res_feat.shape), tuple(pair_feat.shape), spec, id(token))


def _free_bytes(dev):
    """The driver's figure + what torch's caching allocator holds unused: a choice by free memory does not depend on what ran before in this process."""
    return torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)


def _loop_inputs(inputs):
    """(res_feat, pair_feat, mask_generate, mask_res[, aa_allowed][, role]) checked and as the kernels read them (contiguous, features fp32): the caller's own tensors
    where they already are.  aa_allowed, the fifth input of a constrained loop (_LoopSpec.constrained), is the int32 (N, L) tensor of _checked_allowed; role, the last
    input of a guided loop (_LoopSpec.guided), the int32 (N, L) tensor of _checked_role.
    Replicated-complex batches (one crop, N samples: design_for_pdb.py:141-147) may pass the context ONCE: res_feat (1,L,F) / pair_feat (1,L,L,C) are then shared by all
    N samples -- the kernels index pair_feat and its bias cache with batch stride 0, so the 100 x 6 passes over it are served from L2/MALL instead of HBM.  And a test set
    of complexes x S samples may pass G complexes once each: pair_feat (G,L,L,C), samples S c .. S c + S - 1 share entry c (design_for_testset.py:556-589; BASELINE config 4)."""
    res_feat, pair_feat, mask_generate, mask_res, *allowed = inputs
    N, Nc = mask_res.shape[0], pair_feat.shape[0]
    if Nc < 1 or N % Nc:
        raise ValueError(f'pair_feat holds {Nc} complexes for a batch of {N} samples: the batch must be a whole number of samples per complex')
    if res_feat.shape[0] not in (N, Nc):
        raise ValueError('res_feat must hold one entry per sample or one per complex')
    return (res_feat.contiguous().float(), pair_feat.contiguous().float(), mask_generate.contiguous(), mask_res.contiguous(), *(a.contiguous() for a in allowed))


AA_ALL = (1 << 20) - 1          # every residue type: bits 0..19 of an aa_allowed word (include/abopt.h)


def _checked_allowed(aa_allowed, mask_generate):
    """aa_allowed of sample() / optimize() -> None, or the int32 (N, L) tensor the kernels read (bits 20.. cleared).  Accepts (N, L), (1, L) or (L,) int32 / int64, bit k
    of a word = residue type k may be drawn there.  An empty set on a generated residue is refused here, before any launch: one host read per call, outside any captured
    graph (the C ABI defines it -- the type is frozen -- but from Python it is a mistake in building the mask)."""
    if aa_allowed is None:
        return None
    N, L = mask_generate.shape
    a = torch.as_tensor(aa_allowed, device=mask_generate.device)
    if a.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'aa_allowed must be int32 or int64, got {a.dtype}')
    if a.dim() == 1:
        a = a[None]
    if a.dim() != 2 or a.shape[1] != L or a.shape[0] not in (1, N):
        raise ValueError(f'aa_allowed must be ({N}, {L}), (1, {L}) or ({L},), got {tuple(torch.as_tensor(aa_allowed).shape)}')
    a = (a & AA_ALL).to(torch.int32).expand(N, L).contiguous()
    empty = torch.logical_and(mask_generate, a == 0).flatten()
    first = int(torch.where(empty, torch.arange(N * L, device=a.device), N * L).min()) if N * L else 0
    if first < N * L:
        raise ValueError(f'aa_allowed: generated residue {first % L + 1} of sample {first // L} has an empty set of allowed types '
                         '(at least one of bits 0..19 must be set wherever generate_flag is)')
    return a


def _checked_role(guide_role, mask_generate):
    """guide_role of sample() / optimize() -> None, or the int32 (N, L) tensor the guidance kernel reads: bit 0 of a word marks a hotspot, bit 1 a repeller
    (model.guide_roles builds them).  Accepts (N, L), (1, L) or (L,) of any integer dtype.  No device read."""
    if guide_role is None:
        return None
    N, L = mask_generate.shape
    a = torch.as_tensor(guide_role, device=mask_generate.device)
    if a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool:
        raise TypeError(f'guide_role must hold integers (bit 0: hotspot, bit 1: repeller), got {a.dtype}')
    if a.dim() == 1:
        a = a[None]
    if a.dim() != 2 or a.shape[1] != L or a.shape[0] not in (1, N):
        raise ValueError(f'guide_role must be ({N}, {L}), (1, {L}) or ({L},), got {tuple(a.shape)}')
    return a.to(torch.int32).expand(N, L).contiguous()


def _guidance(guide_role, mask_generate, sample_structure, knobs):
    """(role, the guide fields of the _LoopSpec) of sample(guide_role=, guide_attract=, ...) / optimize(...).  The loop is guided iff a role is given and one of the two
    weights is non-zero; otherwise (None, {}): the spec, and so the launches and the graph key, of a call without the keywords.  The knobs are checked either way
    (hip.check_guidance), and guidance of a loop that does not sample the structure is refused: its positions are not the loop's to move.  No device call."""
    kn = hip.check_guidance(**knobs)
    if guide_role is None or (kn['guide_attract'] == 0.0 and kn['guide_repel'] == 0.0):
        return None, {}
    if not sample_structure:
        raise ValueError('guidance moves the generated positions: it needs sample_structure=True (guide_role with a non-zero guide_attract or guide_repel was given)')
    return _checked_role(guide_role, mask_generate), dict(guided=True, **kn)


class FullDPM(_Derived, nn.Module):
    _DERIVED = {'_graphs': collections.OrderedDict, '_graph_seen': set, '_host_sched': type(None)}       # captured loops and host-side caches: per-process objects

    def __init__(self, res_feat_dim, pair_feat_dim, num_steps, eps_net_opt={}, trans_rot_opt={}, trans_pos_opt={},
                 trans_seq_opt={}, position_mean=[0.0, 0.0, 0.0], position_scale=[10.0], obj='pred_noise',
                 num_bins=20, dist_min=0.5, dist_max=19.5, _abdesign=False):
        super().__init__()
        self.abdock = not _abdesign
        self.register_buffer('position_mean', torch.FloatTensor(position_mean).view(1, 1, -1))
        self.register_buffer('position_scale', torch.FloatTensor(position_scale).view(1, 1, -1))
        self.register_buffer('_dummy', torch.empty([0, ]))
        self.eps_net = EpsilonNet(res_feat_dim, pair_feat_dim, **eps_net_opt, no_bins=num_bins if self.abdock else None)
        self.num_steps = num_steps
        self.trans_rot = RotationTransition(num_steps, **trans_rot_opt)
        self.trans_pos = PositionTransition(num_steps, **trans_pos_opt)
        self.trans_seq = AminoacidCategoricalTransition(num_steps, **trans_seq_opt)
        self.obj = obj if self.abdock else 'pred_noise'
        assert self.obj in ['pred_x0', 'pred_noise']
        self.num_bins, self.dist_min, self.dist_max = num_bins, dist_min, dist_max
        if self.abdock:
            self.prmsd = pRMSDCa(num_bins, dist_min=dist_min, dist_max=dist_max)
        self._drop_derived()
        self.graph_mode = 'auto'          # 'auto': eager first, captured from the second call with the same signature; True / False
        self.max_graphs = 4               # captured loops kept (least recently used first out): each pins its own copy of pair_feat, the
                                          # pair-bias cache, the trajectory and a scratch slab -- about 1.2 GB at N=32, L=256

    def clear_graphs(self):
        """Drop every captured loop (and the memory its private pool pins).  Runners that walk many structures of different padded
        lengths can call this between structures; the cache is bounded by `max_graphs` anyway."""
        self._graphs.clear()
        self._graph_seen.clear()

    # ------------------------------------------------------------------ helpers
    def _normalize_position(self, p):
        return (p - self.position_mean) / self.position_scale

    def _unnormalize_position(self, p_norm):
        return p_norm * self.position_scale + self.position_mean

    def _sched_host(self):
        """Schedule scalars as python floats (one D2H at first use; the buffers never change after init)."""
        vs = self.trans_pos.var_sched
        key = (vs.betas.data_ptr(), vs.betas._version)
        if self._host_sched is None or self._host_sched[0] != key:
            g = lambda b: b.detach().cpu().tolist()
            inv = self.trans_rot.angular_distrib_inv
            self._host_sched = (key, dict(
                betas=g(vs.betas), alphas=g(vs.alphas), alpha_bars=g(vs.alpha_bars), sigmas=g(vs.sigmas),
                sr=g(vs.sqrt_recip_alphas_cumprod), srm1=g(vs.sqrt_recipm1_alphas_cumprod),
                std=g(inv.stddevs), approx=g(inv.approx_flag), scale=float(self.position_scale.flatten()[0]),
                mean=g(self.position_mean.flatten())))
        return self._host_sched[1]

    def _stride(self, t, t_prev):
        """(alpha', sigma) of the stride t -> t_prev of a respaced loop, in float64 from the fp32 alpha_bars buffer:
        alpha' = abar_t / abar_u, sigma = sqrt((1 - abar_u) / (1 - abar_t) (1 - alpha')): the DDPM posterior of x_u given x_t and x_0."""
        ab = self._sched_host()['alpha_bars']
        a = ab[t] / ab[t_prev]
        return a, math.sqrt((1.0 - ab[t_prev]) / (1.0 - ab[t]) * (1.0 - a))

    def _step_params(self, t, sample_structure, sample_sequence, ppl_masked, optimize_mode=False, t_prev=None, seq_temperature=1.0, noise_scale=1.0):
        """The scalars of the step t -> t_prev (None: t - 1).  A unit stride reads every one of them from the buffers, as the reference does; a longer one
        computes alpha', sigma and the IGSO(3) width of the stride (_stride) and rounds them once to fp32 -- alpha_bar and the two pred_x0 factors stay those of t.
        seq_temperature / noise_scale: the step is tempered only when one of them differs from 1, so the default step hands the kernels the bytes of every earlier ABI."""
        h = self._sched_host()
        u = t - 1 if t_prev is None else int(t_prev)
        sp = hip.StepParams()
        sp.t, sp.t_prev = t, u
        sp.alpha_bar = h['alpha_bars'][t]
        sp.sqrt_recip_abar, sp.sqrt_recipm1_abar = h['sr'][t], h['srm1'][t]
        if u == t - 1:
            sp.alpha_clamped = max(h['alphas'][t], h['alphas'][-2])
            sp.sigma = h['sigmas'][t]
            sp.igso3_std, sp.igso3_gaussian = h['std'][t], int(h['approx'][t])
        else:
            a, sig = self._stride(t, u)
            sp.alpha_clamped = max(a, h['alphas'][-2])
            sp.sigma = sp.igso3_std = sig
            sp.igso3_gaussian = int(sp.igso3_std <= ctypes.c_float(self.trans_rot.angular_distrib_inv.std_threshold).value)      # fp32 <= fp32, as approx_flag is built
        sp.position_scale = h['scale']
        for k in range(3):
            sp.position_mean[k] = h['mean'][k]
        sp.pred_x0 = int(self.abdock and self.obj == 'pred_x0' and not optimize_mode)
        sp.sample_structure, sp.sample_sequence = int(sample_structure), int(sample_sequence)
        sp.dist_min, sp.dist_max = float(self.dist_min), float(self.dist_max)
        sp.ppl_masked = int(ppl_masked)
        if float(seq_temperature) != 1.0 or float(noise_scale) != 1.0:
            sp.tempered = 1
            sp.seq_temperature = hip.check_temperature('seq_temperature', seq_temperature)
            sp.noise_scale = hip.check_noise_scale('noise_scale', noise_scale)
        return sp

    @staticmethod
    def _loop_steps(spec):
        """[(t, t_prev), ...] of the loop, in the order it runs them: t_start first, 0 last."""
        ts = respaced_steps(spec.t_start, spec.timesteps or None) if isinstance(spec.timesteps, int) else respaced_steps(spec.t_start, timesteps=spec.timesteps)
        return list(zip(ts, ts[1:] + (0,)))

    def _loop_tables(self, pairs):
        """(X rows, cdf rows) of the inverse IGSO(3) histograms, one per step of _loop_steps: the trained rows for unit strides, device-built ones for the sigmas of
        longer strides (RotationTransition.inverse_tables, cached per loop).  Whoever captures the loop keeps the result: the graph's nodes point into it."""
        return self.trans_rot.inverse_tables([t if u == t - 1 else ctypes.c_float(self._stride(t, u)[1]).value for t, u in pairs])

    @staticmethod
    def _new_seed():
        return int(torch.randint(0, 2 ** 62, (1,)).item())

    def _begin(self, seed):
        """What sample() and optimize() start with: the library loaded, a seed from torch's CPU generator unless one is given, the schedule scalars."""
        hip.lib()
        return (self._new_seed() if seed is None else int(seed)), self._sched_host()

    # ------------------------------------------------------------------ training loss
    def forward(self, v_0, p_0, s_0, res_feat, pair_feat, mask_generate, mask_res, denoise_structure, denoise_sequence, t=None, noise=None):
        """dpm_full.py:156-234.  Noising, the denoiser (forward and backward: custom autograd functions over libabopt_hip.so) and the
        rot / pos / seq losses run in HIP kernels (ab_opt_amd/training.py; DESIGN.md section 7 lists what is still an ATen op)."""
        from .training import fulldpm_loss
        return fulldpm_loss(self, v_0, p_0, s_0, res_feat, pair_feat, mask_generate, mask_res, denoise_structure, denoise_sequence, t=t, noise=noise)

    # ------------------------------------------------------------------ sampling
    def _run(self, state, t_start, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence,
             ppl_masked, noise, seed, rng_offset, pbar, stop_after=None, optimize_mode=False, use_bias_cache=None, graph=None, aa_allowed=None):
        """Denoise from step t_start down to 0.  state = (v, p_angstrom, s) on device.  graph: None = self.graph_mode.
        The positional form of benchmarks and tools: the one place that turns such arguments into a _LoopSpec."""
        allowed = _checked_allowed(aa_allowed, mask_generate)
        spec = _LoopSpec(t_start, stop_after, bool(sample_structure), bool(sample_sequence), bool(ppl_masked), bool(optimize_mode), use_bias_cache, allowed is not None)
        return self._denoise(spec, state, self._inputs(res_feat, pair_feat, mask_generate, mask_res, allowed), noise, seed, rng_offset, pbar, graph)

    @staticmethod
    def _inputs(res_feat, pair_feat, mask_generate, mask_res, allowed, role=None):
        """The loop inputs: the four tensors every loop takes, for a constrained one the checked aa_allowed behind them and, for a guided one, the checked role last."""
        return (res_feat, pair_feat, mask_generate, mask_res) + (() if allowed is None else (allowed,)) + (() if role is None else (role,))

    def _denoise(self, spec, state, inputs, noise, seed, rng_offset, pbar, graph=None, range_safe=False):
        """The loop `spec` on inputs = (res_feat, pair_feat, mask_generate, mask_res[, aa_allowed][, role]), eagerly or from its captured graph.  Settles spec.use_bias_cache,
        here and nowhere else.  range_safe: eagerly, the dense layers as fp32 GEMMs (the answer to a raised range guard)."""
        graph = self.graph_mode if graph is None else graph
        res_feat, pair_feat, _, mask_res = inputs[:4]
        capturable = bool(graph) and noise is None and not pbar and not range_safe and res_feat.is_cuda     # (a CPU tensor reaches hip.ptr()'s "no CPU path" error)
        (N, L), Nc = mask_res.shape, pair_feat.shape[0]
        token = self.eps_net.packed() if capturable else None
        cache = spec.use_bias_cache
        if cache is None:
            # shared pair features need the cache; a captured loop with the cache owns its memory already: no need to ask the allocator again (torch.cuda.memory_stats
            # is 0.1 ms of host time per call); a loop that is or will be captured is judged with the graph's own copy of pair_feat on top
            cache = (Nc != N or (capturable and _graph_key(dataclasses.replace(spec, use_bias_cache=True), inputs, token) in self._graphs)
                     or self._bias_cache_fits(Nc, L, res_feat.device, graph=capturable))
        spec = dataclasses.replace(spec, use_bias_cache=bool(cache), query_row_tiles=self._query_row_tiles(spec, inputs[2], bool(cache)))
        key = _graph_key(spec, inputs, token)
        if capturable and key not in self._graphs and graph == 'auto' and key not in self._graph_seen:       # a one-off call should not pay for a capture
            if len(self._graph_seen) >= 64:
                self._graph_seen.clear()
            self._graph_seen.add(key)
            capturable = False
        if not capturable:
            return self._run_eager(spec, state, inputs, noise, seed, rng_offset, pbar, range_safe=range_safe)
        if key not in self._graphs:
            for k in [k for k, g in self._graphs.items() if g.token is not token]:
                del self._graphs[k]                                     # weights were repacked: those graphs point at dead copies
            while len(self._graphs) >= max(1, int(self.max_graphs)):
                self._graphs.popitem(last=False)                        # least recently used: its pool goes back to the allocator
            self._graphs[key] = _LoopGraph(self, spec, state, inputs, token)
        self._graphs.move_to_end(key)
        g = self._graphs[key]
        self.last_run_info = g.info
        return g.replay(state, inputs, seed, rng_offset)

    def _bias_cache_fits(self, n_pair, L, dev, graph=False):
        """The cache costs num_layers * N * L^2 * 48 B next to pair_feat's N * L^2 * 256 B: take it when it fits comfortably
        (a captured graph also keeps its own copy of pair_feat), otherwise the kernels compute the pair bias in place
        (bit-identical, test_pair_bias_cache_is_bit_identical)."""
        if dev.type != 'cuda':
            return False
        need = hip.pair_bias_cache_bytes(n_pair, L, len(self.eps_net.encoder.blocks)) + (hip.pair_terms_bytes(n_pair, L) if L <= 2048 else 0)
        if graph:
            need += n_pair * L * L * 64 * 4
        return need <= _free_bytes(dev) // 2

    def _query_row_tiles(self, spec, mask_generate, cache):
        """_LoopSpec.query_row_tiles of a loop on these masks: ceil(most generated rows of a sample / 16), read from the device once per call and outside any
        capture -- a captured loop's key holds it, so masks that fill more tiles (or fewer) find another graph.  0 where no step of the loop could use a row list:
        the AbDock flavour (its prmsd and perplexity reduce over every row), no pair-bias cache, ABOPT_STEP_COMPACT=0."""
        if spec.query_row_tiles or self.abdock or not cache or not mask_generate.is_cuda or os.environ.get('ABOPT_STEP_COMPACT', '')[:1] == '0':
            return spec.query_row_tiles
        most = int(mask_generate.sum(dim=1).max()) if mask_generate.numel() else 0
        return (most + 15) // 16

    def _pair_terms_wanted(self, N, L, n_pair, dev):
        """The fp16 pair terms pay where the library's launch geometry takes the 32-row block kernels (abopt_pair_terms_used) and their
        n_pair * L^2 * 256 B fit next to everything else; ABOPT_PAIR_TERMS=0 / 1 overrides (0: the fp32 stream everywhere)."""
        e = os.environ.get('ABOPT_PAIR_TERMS')
        if e == '0' or dev.type != 'cuda' or L > 2048 or hip.pair_terms_bytes(n_pair, L) >= (1 << 32):       # (one buffer descriptor addresses the batch's terms)
            return False
        # Measured (profiles/r06_b_pair_terms_ab.txt): the complete term path (pair aggregation + the logits' q . k part) is 8-11 % of a step faster with shared
        # pair features and 7-9 % with distinct ones (the pair aggregation alone bought nothing there: the block kernel then sat on its streams)
        if e != '1' and not hip.pair_terms_used(N, L, N // n_pair if n_pair != N else 0):
            return False
        return hip.pair_terms_bytes(n_pair, L) <= _free_bytes(dev) // 2

    def _run_eager(self, spec, state, inputs, noise, seed, rng_offset, pbar, seed_dev=None, range_safe=False):
        """The loop itself, one C call per step (network evaluation + transitions: hip.eps_net_step); spec.use_bias_cache is settled (_denoise).
        seed_dev: device {seed, offset} (graph capture)."""
        res_feat, pair_feat, mask_generate, mask_res, *extra = _loop_inputs(inputs)
        if len(extra) != int(spec.constrained) + int(spec.guided):
            raise ValueError('a constrained loop takes aa_allowed as its fifth input and a guided one role as its last; a loop that is neither takes four inputs')
        aa_allowed = extra[0] if spec.constrained else None
        role = extra[-1] if spec.guided else None
        if spec.guided and not spec.sample_structure:
            raise ValueError('a loop that does not sample the structure is never guided: its positions are not the loop\'s to move')
        dev = res_feat.device
        N, L = mask_res.shape
        T0, Nc, use_bias_cache = spec.t_start, pair_feat.shape[0], spec.use_bias_cache
        pairs = self._loop_steps(spec)
        K = len(pairs)                                  # slot i of the trajectory buffers holds the state at tau_i: slot K the start, slot 0 the end (slot t in the full loop)
        group = N // Nc
        shared = group > 1
        if shared and not use_bias_cache:
            raise ValueError('a shared pair_feat requires the pair-bias cache')
        if res_feat.shape[0] != N:
            res_feat = res_feat.repeat_interleave(group, dim=0)
        f32 = dict(dtype=torch.float32, device=dev)
        tv = torch.empty(K + 1, N, L, 3, **f32)
        tp = torch.empty(K + 1, N, L, 3, **f32)
        ts = torch.empty(K + 1, N, L, dtype=torch.int64, device=dev)
        tv[K], tp[K], ts[K] = state
        tpr = torch.zeros(K + 1, N, **f32) if self.abdock else None
        tpp = torch.zeros(K + 1, N, **f32) if self.abdock else None
        ew = self.eps_net.packed_fp32() if range_safe else self.eps_net.packed()
        # pair_feat and the weights are constant over the loop: project the pair bias of all blocks once (dpm_full.py:274-283 feeds
        # the same pair_feat to every step); ~0.4 ms at N=32, L=256, outside nothing -- it is part of this call
        pbc = hip.pair_bias_cache(self.eps_net.encoder.packed_array(), len(self.eps_net.encoder.blocks), pair_feat) if use_bias_cache else None
        # ... and, where the 32-row block kernels will run, re-lay pair_feat once as the fp16 operands of their pair aggregation (hip.pair_terms; ~0.25 ms)
        pterms = hip.pair_terms(pair_feat) if (use_bias_cache and self._pair_terms_wanted(N, L, Nc, dev)) else None
        # ... and, for a loop whose spec says how many 16-row tiles its generated rows fill, list them once: the masks are constant over the steps too (hip.query_row_list;
        # inside a captured loop the list is rebuilt by every replay, from the masks the replay copied into the static buffers)
        qrows = (*hip.query_row_list(mask_generate), spec.query_row_tiles) if (spec.query_row_tiles > 0 and use_bias_cache) else None
        X, cdf = self._loop_tables(pairs)
        beta_rows = self.trans_pos.var_sched.betas[:T0 + 1, None].expand(T0 + 1, N).contiguous()    # beta_t per sample, one row per step
        net = dict(v_next=torch.empty(N, L, 3, **f32), R_next=torch.empty(N, L, 3, 3, **f32), eps_pos=torch.empty(N, L, 3, **f32),
                   c=torch.empty(N, L, 20, **f32), prmsd_logits=torch.empty(N, self.num_bins, **f32) if self.abdock else None)
        p_norm = torch.empty(N, L, 3, **f32)
        h_scale, h_mean = self._sched_host()['scale'], self._sched_host()['mean']
        it = enumerate(pairs)
        if pbar:
            from tqdm.auto import tqdm
            it = tqdm(it, total=K, desc='Sampling')
        # dpm_full.py:276: p_t = normalize(traj[t].p) -- here for the first step, afterwards written by the step kernel itself
        torch.sub(tp[K], self.position_mean, out=p_norm).div_(self.position_scale)
        evals = 0
        for j, (t, t_prev) in it:
            if spec.stop_after is not None and j >= spec.stop_after:
                break
            i = K - j                                   # the slot of step t; the step writes slot i - 1, that of t_prev
            # the network is conditioned on the trained beta_t whatever the stride
            out = dict(v=tv[i - 1], p=tp[i - 1], s=ts[i - 1], p_norm=p_norm)
            if self.abdock:
                out.update(prmsd=tpr[i - 1], ppl=tpp[i - 1])
            # Network and transitions as one call: where the library fuses the step's tail, it also runs the mixer of the next evaluation there (carry_out: this call
            # has a next step) and skips its own (carry_in: the previous step of this call left it in the workspace, which nothing else touches inside the loop)
            more = j + 1 < K and (spec.stop_after is None or j + 1 < spec.stop_after)
            # `net` never leaves this function and the transitions keep the old state on context residues: the library may leave it unspecified there
            # (context_outputs_unused; it does where the step's tail is fused, so never with the prmsd head and the perplexity of abdock)
            hip.eps_net_step(ew, tv[i], p_norm, ts[i], res_feat, pair_feat, beta_rows[t], mask_generate, mask_res, self.num_bins, net,
                             self._step_params(t, spec.sample_structure, spec.sample_sequence, spec.ppl_masked, spec.optimize_mode, t_prev,
                                               spec.seq_temperature, spec.noise_scale),
                             noise[t] if noise is not None else None, seed, rng_offset, tp[i], X[j], cdf[j] if noise is None else None, out,
                             pair_bias_cache=pbc, pair_feat_shared=(group if shared else 0), pair_terms=pterms, seed_dev=seed_dev, aa_allowed=aa_allowed,
                             carry_in=j > 0, carry_out=more, context_outputs_unused=True, query_rows=qrows)
            if spec.guided:
                # The nudge of the state the step just stored (p in Angstrom and its normalised copy, the next evaluation's input), the last step included.  The mixer
                # the fused tail carried to the next call reads s_next and v_next only, never the positions: the carry stays valid.  The weights of the step that lands
                # on t_prev: float64 here, rounded once to fp32 at the call, baked into the captured node like every other per-step scalar.
                g = hip.guide_weight(t_prev, self.num_steps, spec.guide_decay)
                hip.guide_positions(tp[i - 1], p_norm, mask_generate, mask_res, role, spec.guide_attract * g, spec.guide_attract_radius, spec.guide_repel * g,
                                    spec.guide_repel_radius, spec.guide_max_shift, h_scale, h_mean)
            evals += 1
        self.last_run_info = dict(bias_cache=use_bias_cache, pair_terms=pterms is not None, shared_context=shared, graph=seed_dev is not None, steps=evals,
                                  query_row_tiles=qrows[2] if qrows else 0, **(dict(guided=True) if spec.guided else {}))
        return tv, tp, ts, tpr, tpp

    def _to_traj(self, T0, tv, tp, ts, tpr, tpp, timesteps=0):
        """Reference layout: dict t -> [v, p, s(, prmsd, ppl)], t>0 on the host, t=0 on the device.  timesteps (a respaced loop's, _LoopSpec.timesteps): the buffers
        hold the visited steps only, slot i the i-th of them from the end, and the dict has those keys."""
        hv, hp, hs = tv[1:].cpu(), tp[1:].cpu(), ts[1:].cpu()       # one bulk D2H each
        traj = {}
        if self.abdock:
            hpr, hpp = tpr.cpu(), tpp.cpu()
        keys = (0,) + tuple(t for t, _ in reversed(self._loop_steps(_LoopSpec(T0, timesteps=timesteps))))        # slot -> step
        for i in range(len(keys) - 1, 0, -1):
            e = [hv[i - 1], hp[i - 1], hs[i - 1]]
            if self.abdock:         # dpm_full.py:269: the first entry carries zeros_like(s) / ones_like(s) in the two extra slots
                e += [torch.zeros_like(e[2]), torch.ones_like(e[2])] if i == len(keys) - 1 else [hpr[i], hpp[i]]
            traj[keys[i]] = e if self.abdock else tuple(e)
        e0 = [tv[0].clone(), tp[0].clone(), ts[0].clone()]       # own storage: the buffers may be a captured graph's static ones
        if self.abdock:
            e0 += [hpr[0], hpp[0]]
        traj[0] = e0 if self.abdock else tuple(e0)
        return traj

    @torch.no_grad()
    def sample(self, v, p, s, res_feat, pair_feat, mask_generate, mask_res, sample_structure=True, sample_sequence=True,
               pbar=False, noise=None, seed=None, rng_offset=0, use_bias_cache=None, graph=None, aa_allowed=None, steps=None, timesteps=None,
               seq_temperature=1.0, noise_scale=1.0, guide_role=None, guide_attract=0.0, guide_attract_radius=8.0, guide_repel=0.0, guide_repel_radius=3.0,
               guide_max_shift=2.0, guide_decay='constant', **kwargs):
        """dpm_full.py:236-302.  `noise` (optional) = {'init': {q4,p,s}, t: {axis,bin,ubin,gauss,z,s_next}} replays
        recorded draws; otherwise a Philox stream seeded from torch's CPU generator is used.
        aa_allowed (optional; no reference counterpart): the residue types that may appear at each generated residue, (N, L) / (1, L) / (L,) int32 or int64 words with
        bit k = type k (model.aa_allowed_mask builds them).  The initial state and every step draw from the allowed types only, so a forbidden type never enters s_t.
        steps = K / timesteps = [...] (optional; no reference counterpart): denoise over a sub-sequence of the trained steps (respaced_steps) --
        K network evaluations instead of num_steps; the trajectory holds the visited steps (and 0) only, and `noise` needs entries for those alone.
        seq_temperature = tau / noise_scale = lambda (optional; no reference counterpart): every step draws its residue types from the
        posterior of the network's prediction at temperature tau (0: greedy; below 1 sharper, above 1 flatter) and adds lambda times the structure noise (0: a
        deterministic structure update).  The initial state is not touched.  With both at 1 the loop is today's, bit for bit; the perplexity of a tau != 1 run
        describes the tempered distribution and is not comparable with one at tau = 1.
        guide_role (optional; no reference counterpart): (N, L) / (1, L) / (L,) integer words, bit 0 = hotspot, bit 1 = repeller
        (model.guide_roles builds them).  After every step the generated residues are pulled, as one rigid set, towards the centroid of the hotspot residues by
        guide_attract (<= 1) times what their centroid's distance exceeds guide_attract_radius, and each is pushed away from the repeller residues closer than
        guide_repel_radius with weight guide_repel; no residue moves more than guide_max_shift per step (all in Angstrom; 8, 3 and 2 are conventional values, not tuned
        ones).  guide_decay 'constant' / 'linear' / 'quadratic': both weights times (u / num_steps)^k for the step that lands on u.  Hotspots and repellers are
        context residues; bits on generated or masked-out residues mean nothing.  Without a role, or with both weights 0, the loop is today's, bit for bit.
        Needs sample_structure=True."""
        tau, lam = hip.check_temperature('seq_temperature', seq_temperature), hip.check_noise_scale('noise_scale', noise_scale)
        role, guide = _guidance(guide_role, mask_generate, sample_structure, dict(
            guide_attract=guide_attract, guide_attract_radius=guide_attract_radius, guide_repel=guide_repel, guide_repel_radius=guide_repel_radius,
            guide_max_shift=guide_max_shift, guide_decay=guide_decay))
        allowed = _checked_allowed(aa_allowed, mask_generate)
        visited = _spec_timesteps(self.num_steps, steps, timesteps)
        seed, h = self._begin(seed)
        state = hip.sample_init(v.float(), p.float(), s, mask_generate, noise['init'] if noise is not None else None, seed, rng_offset,
                                h['scale'], h['mean'], sample_structure, sample_sequence, aa_allowed=allowed)
        spec = _LoopSpec(self.num_steps, None, bool(sample_structure), bool(sample_sequence), ppl_masked=True, use_bias_cache=use_bias_cache,
                         constrained=allowed is not None, timesteps=visited, seq_temperature=tau, noise_scale=lam, **guide)
        inputs = self._inputs(res_feat, pair_feat, mask_generate, mask_res, allowed, role)
        return self._to_traj(spec.t_start, *_range_guarded(lambda safe: self._denoise(spec, state, inputs, noise, seed, rng_offset, pbar, graph, safe)), timesteps=visited)

    @torch.no_grad()
    def optimize(self, v, p, s, opt_step, res_feat, pair_feat, mask_generate, mask_res, sample_structure=True,
                 sample_sequence=True, pbar=False, noise=None, seed=None, rng_offset=0, use_bias_cache=None, graph=None, aa_allowed=None, steps=None, timesteps=None,
                 seq_temperature=1.0, noise_scale=1.0, guide_role=None, guide_attract=0.0, guide_attract_radius=8.0, guide_repel=0.0, guide_repel_radius=3.0,
                 guide_max_shift=2.0, guide_decay='constant'):
        """dpm_full.py:304-367: noise the input to step `opt_step`, then denoise.  aa_allowed: as in sample(); the forward noising draws from the allowed types too.
        steps = K / timesteps: as in sample(), over [0, opt_step] (K <= opt_step).  seq_temperature / noise_scale: as in sample(), on the denoising steps; the
        forward noising to opt_step is not touched.  guide_role and the guide_* knobs: as in sample(), behind every denoising step; the step weight of
        guide_decay counts in the model's num_steps, not in opt_step."""
        tau, lam = hip.check_temperature('seq_temperature', seq_temperature), hip.check_noise_scale('noise_scale', noise_scale)
        role, guide = _guidance(guide_role, mask_generate, sample_structure, dict(
            guide_attract=guide_attract, guide_attract_radius=guide_attract_radius, guide_repel=guide_repel, guide_repel_radius=guide_repel_radius,
            guide_max_shift=guide_max_shift, guide_decay=guide_decay))
        allowed = _checked_allowed(aa_allowed, mask_generate)
        visited = _spec_timesteps(opt_step, steps, timesteps)
        seed, h = self._begin(seed)
        N = v.shape[0]
        t = torch.full([N], opt_step, dtype=torch.long, device=res_feat.device)
        init_noise = noise.get('init') if noise is not None else None
        # dpm_full.py:320-339: noise structure and/or sequence to step opt_step (position in Angstrom in and out)
        state = hip.add_noise(t, self.trans_pos.var_sched.alpha_bars, self.trans_rot.angular_distrib_fwd, init_noise, seed, rng_offset,
                              v.float(), p.float(), s, mask_generate, h['scale'], h['mean'],
                              noise_structure=sample_structure, noise_sequence=sample_sequence, grad_mode=False, aa_allowed=allowed)
        state = (state[0], state[1], torch.where(mask_generate, state[2], s))       # dpm_full.py:335
        # dpm_full.py:351-358: the loop feeds the net's third output to the position update as noise whatever `obj` is,
        # and averages the perplexity over all residues (calc_perplexity(logits) without a mask)
        spec = _LoopSpec(opt_step, None, bool(sample_structure), bool(sample_sequence), ppl_masked=False, optimize_mode=True, use_bias_cache=use_bias_cache,
                         constrained=allowed is not None, timesteps=visited, seq_temperature=tau, noise_scale=lam, **guide)
        inputs = self._inputs(res_feat, pair_feat, mask_generate, mask_res, allowed, role)
        # same counters as add_noise, other sub-sequence tags (csrc/denoise.hip): a sample's stream position does not depend on the batch it sits in
        traj = self._to_traj(opt_step, *_range_guarded(lambda safe: self._denoise(spec, state, inputs, noise, seed, rng_offset, pbar, graph, safe)), timesteps=visited)
        return {k: tuple(e) for k, e in traj.items()}


class _LoopGraph:
    """One captured denoising loop: static copies of the inputs, the hipGraph, and the trajectory buffers it writes.

    Capture runs FullDPM._run_eager under torch.cuda.graph(): every launch of libabopt_hip.so goes to torch's current stream, which
    is the capturing stream, and every tensor the loop allocates (trajectory, network outputs, pair-bias cache, workspace) comes from
    the graph's private pool and keeps its address across replays.  Nothing in the loop reads device memory on the host."""

    def __init__(self, dpm, spec, state, inputs, token):
        self.token = token                                              # EpsilonNet.packed() at capture: keeps the packed weights this graph points at alive
        self.state = tuple(a.clone() for a in state)
        static = tuple(a.clone() for a in _loop_inputs(inputs))
        self.res_feat, self.pair_feat, self.mask_generate, self.mask_res = static[:4]
        self.aa_allowed = static[4] if spec.constrained else None      # a constrained loop's mask is an input like mask_generate: refreshed before each replay
        self.role = static[-1] if spec.guided else None                # and so are a guided loop's roles
        self.seed_dev = torch.zeros(2, dtype=torch.int64, device=self.res_feat.device)
        self.tables = dpm._loop_tables(dpm._loop_steps(spec))          # the IGSO(3) rows the captured steps read: the cache that built them may drop them, this graph may not
        run = lambda stop_after: dpm._run_eager(dataclasses.replace(spec, stop_after=stop_after), self.state, static, None, 0, 0, False, seed_dev=self.seed_dev)
        hip.prof_enable(False)
        run(1)                                                          # warm: kernel attributes, host-side caches, cdf tables
        torch.cuda.synchronize(self.res_feat.device)
        self.graph = torch.cuda.CUDAGraph()
        hip.prof_enable(hip.GRAPH_CAPTURE_EVENTS)                       # normally off: the measurement hook's event pairs stay out of the graph
        if hip.GRAPH_CAPTURE_SPANS:
            hip.lib().abopt_prof_enable(3)               # span slots for the dominant kernel's launches, baked into the captured nodes
        try:
            # the scratch slab the capture allocates on the capturing stream lives in this graph's pool: this graph keeps it, it serves no other stream user,
            # and the capture uses no slab that an earlier capture left under the capturing stream's key (hip.Workspace.private says why)
            with hip.Workspace.private() as self.keep, torch.cuda.graph(self.graph):
                self.out = run(spec.stop_after)
        finally:
            if hip.GRAPH_CAPTURE_EVENTS:
                hip.lib().abopt_prof_enable(2)           # stop bracketing launches, keep the pairs the graph re-records
            if hip.GRAPH_CAPTURE_SPANS:
                hip.lib().abopt_prof_enable(4)
        self.info = dict(dpm.last_run_info)
        self._pf_src = None                                             # (weakref to the caller's pair_feat, its _version) of the last copy

    def replay(self, state, inputs, seed, rng_offset):
        res_feat, pair_feat, mask_generate, mask_res, *extra = inputs
        for dst, src in zip(self.state, state):
            dst.copy_(src)
        self.res_feat.copy_(res_feat if res_feat.shape == self.res_feat.shape else res_feat.expand_as(self.res_feat))
        # pair_feat is the one large input (537 MB at N=32, L=256): when the caller hands over the very tensor object of the last replay,
        # unmodified (same _version), the static copy is still current.  Identity of the live OBJECT, not of the address: a freed tensor's
        # address can come back from the allocator with other contents.
        # `_version` counts autograd-visible in-place writes only: a caller that refreshes the SAME tensor object through raw pointers
        # (this library's kernels writing into it, `.data`) must pass a new tensor object or call clear_graphs(); inference-mode tensors
        # have no version counter at all and are always copied.
        src = self._pf_src
        try:
            ver = pair_feat._version
        except RuntimeError:
            ver = None
        same = ver is not None and src is not None and src[0]() is pair_feat and src[1] == ver
        if not same and pair_feat.data_ptr() != self.pair_feat.data_ptr():
            self.pair_feat.copy_(pair_feat)
            self._pf_src = (weakref.ref(pair_feat), ver) if ver is not None else None
        self.mask_generate.copy_(mask_generate)
        self.mask_res.copy_(mask_res)
        if self.aa_allowed is not None:
            self.aa_allowed.copy_(extra[0])
        if self.role is not None:
            self.role.copy_(extra[-1])
        self.seed_dev.copy_(torch.tensor([int(seed), int(rng_offset)], dtype=torch.int64))
        self.graph.replay()
        return self.out
