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
import weakref
import os
import torch
import torch.nn as nn

from . import hip
from .modules import (EpsilonNet, RotationTransition, PositionTransition, AminoacidCategoricalTransition, pRMSDCa)


class FullDPM(nn.Module):

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
        self._host_sched = None
        self._graphs, self._graph_seen = collections.OrderedDict(), set()
        self.graph_mode = 'auto'          # 'auto': eager first, captured from the second call with the same signature; True / False
        self.max_graphs = 4               # captured loops kept (least recently used first out): each pins its own copy of pair_feat, the
                                          # pair-bias cache, the trajectory and a scratch slab -- about 1.2 GB at N=32, L=256

    def __getstate__(self):
        """Captured graphs and host-side caches are per-process objects: a pickled / deep-copied model starts without them."""
        d = dict(self.__dict__)
        d['_graphs'], d['_graph_seen'], d['_host_sched'] = collections.OrderedDict(), set(), None
        return d

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

    def _step_params(self, t, sample_structure, sample_sequence, ppl_masked, optimize_mode=False):
        h = self._sched_host()
        sp = hip.StepParams()
        sp.t = t
        sp.alpha_clamped = max(h['alphas'][t], h['alphas'][-2])
        sp.alpha_bar, sp.sigma = h['alpha_bars'][t], h['sigmas'][t]
        sp.sqrt_recip_abar, sp.sqrt_recipm1_abar = h['sr'][t], h['srm1'][t]
        sp.igso3_std, sp.igso3_gaussian = h['std'][t], int(h['approx'][t])
        sp.position_scale = h['scale']
        for k in range(3):
            sp.position_mean[k] = h['mean'][k]
        sp.pred_x0 = int(self.abdock and self.obj == 'pred_x0' and not optimize_mode)
        sp.sample_structure, sp.sample_sequence = int(sample_structure), int(sample_sequence)
        sp.dist_min, sp.dist_max = float(self.dist_min), float(self.dist_max)
        sp.ppl_masked = int(ppl_masked)
        return sp

    @staticmethod
    def _new_seed():
        return int(torch.randint(0, 2 ** 62, (1,)).item())

    # ------------------------------------------------------------------ training loss
    def forward(self, v_0, p_0, s_0, res_feat, pair_feat, mask_generate, mask_res, denoise_structure, denoise_sequence, t=None, noise=None):
        """dpm_full.py:156-234.  Noising, the denoiser (forward and backward: custom autograd functions over libabopt_hip.so) and the
        rot / pos / seq losses run in HIP kernels (ab_opt_amd/training.py; DESIGN.md section 7 lists what is still an ATen op)."""
        from .training import fulldpm_loss
        return fulldpm_loss(self, v_0, p_0, s_0, res_feat, pair_feat, mask_generate, mask_res, denoise_structure, denoise_sequence, t=t, noise=noise)

    # ------------------------------------------------------------------ sampling
    def _run(self, state, t_start, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence,
             ppl_masked, noise, seed, rng_offset, pbar, stop_after=None, optimize_mode=False, use_bias_cache=None, graph=None):
        """Denoise from step t_start down to 0.  state = (v, p_angstrom, s) on device.  graph: None = self.graph_mode."""
        graph = self.graph_mode if graph is None else graph
        if noise is not None or pbar or not graph or not res_feat.is_cuda:     # (a CPU tensor reaches hip.ptr()'s "no CPU path" error)
            return self._run_eager(state, t_start, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence,
                                   ppl_masked, noise, seed, rng_offset, pbar, stop_after, optimize_mode, use_bias_cache)
        N, L = mask_res.shape
        shared = pair_feat.shape[0] != N
        self.eps_net.packed()
        mk = lambda cache: (res_feat.device.index, N, L, t_start, stop_after, bool(sample_structure), bool(sample_sequence), bool(ppl_masked),
                            bool(optimize_mode), tuple(res_feat.shape), tuple(pair_feat.shape), bool(cache), id(self.eps_net._pack))
        if use_bias_cache is None:
            # a captured loop with the cache owns its memory already: no need to ask the allocator again (torch.cuda.memory_stats is 0.1 ms of host time per call)
            use_bias_cache = shared or mk(True) in self._graphs or self._bias_cache_fits(pair_feat.shape[0], L, res_feat.device, graph=True)
        key = mk(use_bias_cache)
        g = self._graphs.get(key)
        if g is None:
            if graph == 'auto' and key not in self._graph_seen:         # a one-off call should not pay for a capture
                if len(self._graph_seen) >= 64:
                    self._graph_seen.clear()
                self._graph_seen.add(key)
                return self._run_eager(state, t_start, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence,
                                       ppl_masked, noise, seed, rng_offset, pbar, stop_after, optimize_mode, use_bias_cache)
            for k in [k for k, v in self._graphs.items() if v.pack is not self.eps_net._pack]:
                del self._graphs[k]                                     # weights were repacked: those graphs point at dead copies
            while len(self._graphs) >= max(1, int(self.max_graphs)):
                self._graphs.popitem(last=False)                        # least recently used: its pool goes back to the allocator
            g = self._graphs[key] = _LoopGraph(self, state, t_start, res_feat, pair_feat, mask_generate, mask_res, sample_structure,
                                               sample_sequence, ppl_masked, stop_after, optimize_mode, use_bias_cache)
        self._graphs.move_to_end(key)
        self.last_run_info = g.info
        return g.replay(state, res_feat, pair_feat, mask_generate, mask_res, seed, rng_offset)

    def _bias_cache_fits(self, n_pair, L, dev, graph=False):
        """The cache costs num_layers * N * L^2 * 48 B next to pair_feat's N * L^2 * 256 B: take it when it fits comfortably
        (a captured graph also keeps its own copy of pair_feat), otherwise the kernels compute the pair bias in place
        (bit-identical, test_pair_bias_cache_is_bit_identical).  Free = what the driver reports + what torch's caching allocator
        holds but is not using, so the choice does not depend on what ran before in this process."""
        if dev.type != 'cuda':
            return False
        need = hip.pair_bias_cache_bytes(n_pair, L, len(self.eps_net.encoder.blocks)) + (hip.pair_terms_bytes(n_pair, L) if L <= 2048 else 0)
        if graph:
            need += n_pair * L * L * 64 * 4
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        return need <= free // 2

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
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        return hip.pair_terms_bytes(n_pair, L) <= free // 2

    def _run_eager(self, state, t_start, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence,
                   ppl_masked, noise, seed, rng_offset, pbar, stop_after=None, optimize_mode=False, use_bias_cache=None, seed_dev=None, range_safe=False):
        """The loop itself, one C call per network evaluation and one per transition.  seed_dev: device {seed, offset} (graph capture).
        range_safe: the dense layers as fp32 GEMMs (the answer to a raised range guard, _guarded)."""
        dev = res_feat.device
        N, L = mask_res.shape
        T0 = t_start
        f32 = dict(dtype=torch.float32, device=dev)
        tv = torch.empty(T0 + 1, N, L, 3, **f32)
        tp = torch.empty(T0 + 1, N, L, 3, **f32)
        ts = torch.empty(T0 + 1, N, L, dtype=torch.int64, device=dev)
        tv[T0], tp[T0], ts[T0] = state
        tpr = torch.zeros(T0 + 1, N, **f32) if self.abdock else None
        tpp = torch.zeros(T0 + 1, N, **f32) if self.abdock else None

        # Replicated-complex batches (one crop, N samples: design_for_pdb.py:141-147) may pass the context ONCE: res_feat
        # (1,L,F) / pair_feat (1,L,L,C) are then shared by all N samples -- the kernels index pair_feat and its bias cache
        # with batch stride 0, so the 100 x 6 passes over it are served from L2/MALL instead of HBM.
        # ... and a test set of complexes x S samples may pass G complexes once each: pair_feat (G,L,L,C), samples S c .. S c + S - 1 share
        # entry c (design_for_testset.py:556-589 runs them one structure at a time; BASELINE config 4).
        Nc = pair_feat.shape[0]
        if Nc < 1 or N % Nc:
            raise ValueError(f'pair_feat holds {Nc} complexes for a batch of {N} samples: the batch must be a whole number of samples per complex')
        group = N // Nc
        shared = group > 1
        if use_bias_cache is None:
            use_bias_cache = shared or self._bias_cache_fits(Nc, L, dev)
        if shared and not use_bias_cache:
            raise ValueError('a shared pair_feat requires the pair-bias cache')
        if res_feat.shape[0] != N:
            if res_feat.shape[0] != Nc:
                raise ValueError('res_feat must hold one entry per sample or one per complex')
            res_feat = res_feat.repeat_interleave(group, dim=0)
        res_feat, pair_feat = res_feat.contiguous().float(), pair_feat.contiguous().float()
        mask_generate, mask_res = mask_generate.contiguous(), mask_res.contiguous()
        ew = self.eps_net.packed_fp32() if range_safe else self.eps_net.packed()
        # pair_feat and the weights are constant over the loop: project the pair bias of all blocks once (dpm_full.py:274-283 feeds
        # the same pair_feat to every step); ~0.4 ms at N=32, L=256, outside nothing -- it is part of this call
        pbc = hip.pair_bias_cache(self.eps_net.encoder.packed_array(), len(self.eps_net.encoder.blocks), pair_feat) if use_bias_cache else None
        # ... and, where the 32-row block kernels will run, re-lay pair_feat once as the fp16 operands of their pair aggregation (hip.pair_terms; ~0.25 ms)
        pterms = hip.pair_terms(pair_feat) if (use_bias_cache and self._pair_terms_wanted(N, L, Nc, dev)) else None
        h = self._sched_host()
        inv = self.trans_rot.angular_distrib_inv
        X, cdf = inv.X, (inv.cdf() if noise is None else None)
        beta_rows = self.trans_pos.var_sched.betas[:T0 + 1, None].expand(T0 + 1, N).contiguous()    # beta_t per sample, one row per step
        net = dict(v_next=torch.empty(N, L, 3, **f32), R_next=torch.empty(N, L, 3, 3, **f32), eps_pos=torch.empty(N, L, 3, **f32),
                   c=torch.empty(N, L, 20, **f32), prmsd_logits=torch.empty(N, self.num_bins, **f32) if self.abdock else None)
        p_norm = torch.empty(N, L, 3, **f32)
        scale, mean = self.position_scale, self.position_mean
        it = range(T0, 0, -1)
        if pbar:
            from tqdm.auto import tqdm
            it = tqdm(it, total=T0, desc='Sampling')
        # dpm_full.py:276: p_t = normalize(traj[t].p) -- here for the first step, afterwards written by the step kernel itself
        torch.sub(tp[T0], mean, out=p_norm).div_(scale)
        for t in it:
            if stop_after is not None and T0 - t >= stop_after:
                break
            beta = beta_rows[t]
            hip.eps_net_forward(ew, tv[t], p_norm, ts[t], res_feat, pair_feat, beta, mask_generate, mask_res,
                                self.abdock, self.num_bins, False, out=net, pair_bias_cache=pbc, pair_feat_shared=(group if shared else 0), pair_terms=pterms)
            sp = self._step_params(t, sample_structure, sample_sequence, ppl_masked, optimize_mode)
            out = dict(v=tv[t - 1], p=tp[t - 1], s=ts[t - 1], p_norm=p_norm)
            if self.abdock:
                out.update(prmsd=tpr[t - 1], ppl=tpp[t - 1])
            hip.denoise_step(sp, noise[t] if noise is not None else None, seed, rng_offset,
                             tv[t], tp[t], ts[t], net['v_next'], net['eps_pos'], net['c'], net['prmsd_logits'], mask_generate,
                             X[t], cdf[t] if cdf is not None else None, self.num_bins, out, seed_dev=seed_dev)
        self.last_run_info = dict(bias_cache=bool(use_bias_cache), pair_terms=pterms is not None, shared_context=bool(shared), graph=seed_dev is not None)
        return tv, tp, ts, tpr, tpp

    def _guarded(self, run, rerun):
        """Range guard of the two-term fp16 layers (include/abopt.h: abopt_nonfinite_flag): the reference's fp32 layers take activations beyond 65504, the
        fp16 terms do not (inf -> NaN in the heads' outputs, which raises a device flag).  One flag read per call; if it is up, the whole loop is repeated
        with the dense layers as fp32 GEMMs -- the caller gets what the reference's arithmetic gives (NaN only where fp32 itself overflows)."""
        hip.nonfinite_flag_reset()                   # in stream order, no synchronisation: the flag read below is this call's
        out = run()
        if hip.nonfinite_flag(reset=False):
            import warnings
            warnings.warn('ab_opt_amd: a denoiser activation left the fp16 range (|x| >= 65504) or an input was not finite; this call is repeated with '
                          'the dense layers as fp32 GEMMs (slower, fp32 range)', RuntimeWarning, stacklevel=3)
            out = rerun()
            hip.nonfinite_flag_reset()
        return out

    def _to_traj(self, T0, tv, tp, ts, tpr, tpp, first_extra):
        """Reference layout: dict t -> [v, p, s(, prmsd, ppl)], t>0 on the host, t=0 on the device."""
        hv, hp, hs = tv[1:].cpu(), tp[1:].cpu(), ts[1:].cpu()       # one bulk D2H each
        traj = {}
        if self.abdock:
            hpr, hpp = tpr.cpu(), tpp.cpu()
        for t in range(T0, 0, -1):
            e = [hv[t - 1], hp[t - 1], hs[t - 1]]
            if self.abdock:
                e += list(first_extra(hs[t - 1])) if t == T0 else [hpr[t], hpp[t]]
            traj[t] = e if self.abdock else tuple(e)
        e0 = [tv[0].clone(), tp[0].clone(), ts[0].clone()]       # own storage: the buffers may be a captured graph's static ones
        if self.abdock:
            e0 += [hpr[0], hpp[0]]
        traj[0] = e0 if self.abdock else tuple(e0)
        return traj

    @torch.no_grad()
    def sample(self, v, p, s, res_feat, pair_feat, mask_generate, mask_res, sample_structure=True, sample_sequence=True,
               pbar=False, noise=None, seed=None, rng_offset=0, use_bias_cache=None, graph=None, **kwargs):
        """dpm_full.py:236-302.  `noise` (optional) = {'init': {q4,p,s}, t: {axis,bin,ubin,gauss,z,s_next}} replays
        recorded draws; otherwise a Philox stream seeded from torch's CPU generator is used."""
        hip.lib()
        seed = self._new_seed() if seed is None else int(seed)
        h = self._sched_host()
        state = hip.sample_init(v.float(), p.float(), s, mask_generate, noise['init'] if noise is not None else None, seed, rng_offset,
                                h['scale'], h['mean'], sample_structure, sample_sequence)
        T = self.num_steps
        out = self._guarded(lambda: self._run(state, T, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence, True,
                                              noise, seed, rng_offset, pbar, use_bias_cache=use_bias_cache, graph=graph),
                            lambda: self._run_eager(state, T, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence, True,
                                                    noise, seed, rng_offset, pbar, use_bias_cache=use_bias_cache, range_safe=True))
        # dpm_full.py:269: the first entry carries zeros_like(s) / ones_like(s) in the two extra slots
        return self._to_traj(T, *out, first_extra=lambda s_: (torch.zeros_like(s_), torch.ones_like(s_)))

    @torch.no_grad()
    def optimize(self, v, p, s, opt_step, res_feat, pair_feat, mask_generate, mask_res, sample_structure=True,
                 sample_sequence=True, pbar=False, noise=None, seed=None, rng_offset=0, use_bias_cache=None, graph=None):
        """dpm_full.py:304-367: noise the input to step `opt_step`, then denoise."""
        hip.lib()
        seed = self._new_seed() if seed is None else int(seed)
        h = self._sched_host()
        N = v.shape[0]
        t = torch.full([N], opt_step, dtype=torch.long, device=res_feat.device)
        init_noise = noise.get('init') if noise is not None else None
        # dpm_full.py:320-339: noise structure and/or sequence to step opt_step (position in Angstrom in and out)
        state = hip.add_noise(t, self.trans_pos.var_sched.alpha_bars, self.trans_rot.angular_distrib_fwd, init_noise, seed, rng_offset,
                              v.float(), p.float(), s, mask_generate, h['scale'], h['mean'],
                              noise_structure=sample_structure, noise_sequence=sample_sequence, grad_mode=False)
        state = (state[0], state[1], torch.where(mask_generate, state[2], s))       # dpm_full.py:335
        # dpm_full.py:351-358: the loop feeds the net's third output to the position update as noise whatever `obj` is,
        # and averages the perplexity over all residues (calc_perplexity(logits) without a mask)
        out = self._guarded(lambda: self._run(state, opt_step, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence, False,
                                              noise, seed, rng_offset, pbar, optimize_mode=True, use_bias_cache=use_bias_cache, graph=graph),
                            lambda: self._run_eager(state, opt_step, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence, False,
                                                    noise, seed, rng_offset, pbar, optimize_mode=True, use_bias_cache=use_bias_cache, range_safe=True))     # same counters as add_noise, other sub-sequence tags (csrc/denoise.hip): a sample's stream position does not depend on the batch it sits in
        traj = self._to_traj(opt_step, *out, first_extra=lambda s_: (torch.zeros_like(s_), torch.ones_like(s_)))
        return {k: tuple(e) for k, e in traj.items()}


class _LoopGraph:
    """One captured denoising loop: static copies of the inputs, the hipGraph, and the trajectory buffers it writes.

    Capture runs FullDPM._run_eager under torch.cuda.graph(): every launch of libabopt_hip.so goes to torch's current stream, which
    is the capturing stream, and every tensor the loop allocates (trajectory, network outputs, pair-bias cache, workspace) comes from
    the graph's private pool and keeps its address across replays.  Nothing in the loop reads device memory on the host."""

    def __init__(self, dpm, state, t_start, res_feat, pair_feat, mask_generate, mask_res, sample_structure, sample_sequence, ppl_masked,
                 stop_after, optimize_mode, use_bias_cache):
        dev = res_feat.device
        self.pack = dpm.eps_net._pack                                   # keeps the packed weights this graph points at alive
        self.state = tuple(a.clone() for a in state)
        self.res_feat, self.pair_feat = res_feat.contiguous().float().clone(), pair_feat.contiguous().float().clone()
        self.mask_generate, self.mask_res = mask_generate.contiguous().clone(), mask_res.contiguous().clone()
        self.seed_dev = torch.zeros(2, dtype=torch.int64, device=dev)
        args = (self.state, t_start, self.res_feat, self.pair_feat, self.mask_generate, self.mask_res, sample_structure, sample_sequence,
                ppl_masked, None, 0, 0, False)
        kw = dict(optimize_mode=optimize_mode, use_bias_cache=use_bias_cache, seed_dev=self.seed_dev)
        hip.prof_enable(False)
        dpm._run_eager(*args, stop_after=1, **kw)                       # warm: kernel attributes, host-side caches, cdf tables
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        before = set(hip.Workspace._bufs)
        hip.prof_enable(hip.GRAPH_CAPTURE_EVENTS)                       # normally off: the measurement hook's event pairs stay out of the graph
        if hip.GRAPH_CAPTURE_SPANS:
            hip.lib().abopt_prof_enable(3)               # span slots for the dominant kernel's launches, baked into the captured nodes
        try:
            with torch.cuda.graph(self.graph):
                self.out = dpm._run_eager(*args, stop_after=stop_after, **kw)
        finally:
            if hip.GRAPH_CAPTURE_EVENTS:
                hip.lib().abopt_prof_enable(2)           # stop bracketing launches, keep the pairs the graph re-records
            if hip.GRAPH_CAPTURE_SPANS:
                hip.lib().abopt_prof_enable(4)
        # the scratch slab the capture allocated on the capturing stream lives in this graph's pool: it must not serve another stream user
        self.keep = [hip.Workspace._bufs.pop(k) for k in set(hip.Workspace._bufs) - before]
        self.info = dict(dpm.last_run_info)
        self._pf_src = None                                             # (weakref to the caller's pair_feat, its _version) of the last copy

    def replay(self, state, res_feat, pair_feat, mask_generate, mask_res, seed, rng_offset):
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
        self.seed_dev.copy_(torch.tensor([int(seed), int(rng_offset)], dtype=torch.int64))
        self.graph.replay()
        return self.out
