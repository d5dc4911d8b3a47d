"""ctypes binding of libabopt_hip.so (the C ABI in include/abopt.h).

PyTorch is used only as the owner of device memory and streams: every call passes
`tensor.data_ptr()` and `torch.cuda.current_stream().cuda_stream`.  There is no fallback:
if the library is missing or a tensor is not on a HIP device, these functions raise.
"""
import contextlib
import ctypes as C
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_longlong, c_size_t, c_uint64, c_void_p
import os
import threading
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ABOPT_LIB_PATH: developer override to load a variant build of the same ABI (csrc/Makefile VARIANT=...: A/B of two source trees)
LIB_PATH = os.environ.get('ABOPT_LIB_PATH') or os.path.join(_HERE, 'libabopt_hip.so')
ABI_VERSION = 59

c_f = C.c_void_p        # device float*
c_i64 = C.c_void_p      # device int64*
c_u8 = C.c_void_p       # device uint8*


class GemmTnProblem(C.Structure):
    """abopt_gemm_tn_problem (include/abopt.h)"""
    _fields_ = [('a', C.c_void_p), ('b', C.c_void_p), ('c', C.c_void_p), ('lda', C.c_int), ('ldb', C.c_int), ('m', C.c_int), ('n', C.c_int), ('k', C.c_int)]


class GaWeights(C.Structure):
    _fields_ = [(n, c_f) for n in (
        'w_node', 'w_pair_bias', 'spatial_coef', 'w_out', 'b_out', 'ln1_gamma', 'ln1_beta',
        'w_mlp0', 'b_mlp0', 'w_mlp1', 'b_mlp1', 'w_mlp2', 'b_mlp2', 'ln2_gamma', 'ln2_beta', 'w_node_frag', 'w_out_frag', 'w_mlp_frag', 'w_out_terms')]


class GaDebug(C.Structure):
    _fields_ = [('logits', c_f), ('alpha', c_f), ('feat', c_f)]


class EpsWeights(C.Structure):
    _fields_ = ([(n, c_f) for n in ('seq_embed', 'w_mix0', 'b_mix0', 'w_mix1', 'b_mix1')] +
                [('blocks', C.POINTER(GaWeights)), ('num_layers', C.c_int)] +
                [(n, c_f) for n in ('w_head1', 'b_head1', 'w_crd2', 'b_crd2', 'w_crd3', 'b_crd3',
                                    'w_rot2', 'b_rot2', 'w_rot3', 'b_rot3', 'w_seq2', 'b_seq2', 'w_seq3', 'b_seq3',
                                    'prmsd_ln_gamma', 'prmsd_ln_beta', 'w_prmsd1', 'b_prmsd1', 'w_prmsd2', 'b_prmsd2',
                                    'w_prmsd3', 'b_prmsd3')] +
                [('num_bins', C.c_int), ('w_heads_frag', c_f), ('w_mix_frag', c_f), ('mix_table', c_f)])


class EncodeInputs(C.Structure):
    _fields_ = ([('N', C.c_int), ('L', C.c_int), ('atoms_in', C.c_int), ('atoms', C.c_int)] +
                [(n, C.c_void_p) for n in ('aa', 'res_nb', 'chain_nb', 'fragment_type', 'hotspot', 'pos_atoms', 'mask_atoms',
                                           'structure_mask', 'sequence_mask')])


class ResidueEmbedWeights(C.Structure):
    _fields_ = [(n, c_f) for n in ('aatype_embed', 'type_embed', 'hotspot_embed', 'freq_bands', 'w0', 'b0', 'w1', 'b1', 'w2', 'b2', 'w3', 'b3')]


class PairEmbedWeights(C.Structure):
    _fields_ = [(n, c_f) for n in ('aa_pair_embed', 'relpos_embed', 'aapair_to_distcoef', 'freq_bands', 'wd0', 'bd0', 'wd1', 'bd1',
                                   'wo0', 'bo0', 'wo1', 'bo1', 'wo2', 'bo2')]


class StepParams(C.Structure):
    _fields_ = [('t', C.c_int), ('alpha_clamped', C.c_float), ('alpha_bar', C.c_float), ('sigma', C.c_float),
                ('sqrt_recip_abar', C.c_float), ('sqrt_recipm1_abar', C.c_float), ('igso3_std', C.c_float),
                ('igso3_gaussian', C.c_int), ('position_scale', C.c_float), ('position_mean', C.c_float * 3),
                ('pred_x0', C.c_int), ('sample_structure', C.c_int), ('sample_sequence', C.c_int),
                ('dist_min', C.c_float), ('dist_max', C.c_float), ('ppl_masked', C.c_int), ('t_prev', C.c_int),
                ('tempered', C.c_int), ('seq_temperature', C.c_float), ('noise_scale', C.c_float)]


class AddNoiseNoise(C.Structure):
    _fields_ = [('axis', c_f), ('bin', c_i64), ('ubin', c_f), ('gauss', c_f), ('pos', c_f), ('s_noisy', c_i64)]


class StepNoise(C.Structure):
    _fields_ = [('axis', c_f), ('bin', c_i64), ('ubin', c_f), ('gauss', c_f), ('z', c_f), ('s_next', c_i64)]


c_i32 = C.c_void_p      # device int32*
c_stream = C.c_void_p   # abopt_stream (a hipStream_t)

# The one Python statement of the C ABI: name -> (restype, argtypes) of every function of include/abopt.h, in the header's order, each entry reading
# like its prototype (tests/test_abi.py::test_binding_signatures_match_header holds it to the header).  Device and host data pointers are c_void_p (the
# aliases above name what a device pointer points to); pointer-to-pointer parameters and host arrays (adam's numel, position_mean) are c_void_p too and
# take the ctypes arrays the wrappers build; `const abopt_X*` is POINTER of the mirror; int* / double* / long long* are host out-parameters.
_SIGNATURES = {
    'abopt_abi_version': (c_int, []),
    'abopt_last_error': (c_char_p, []),
    'abopt_device_info': (c_int, [POINTER(c_int), POINTER(c_int), c_char_p, c_int]),
    'abopt_so3_exp': (c_int, [c_f, c_f, c_int64, c_stream]),
    'abopt_so3_log': (c_int, [c_f, c_f, c_int64, c_int, c_stream]),
    'abopt_node_frag_source_row': (c_int, [c_int, c_int, c_int]),
    'abopt_node_frag_floats': (c_size_t, []),
    'abopt_out_frag_floats': (c_size_t, []),
    'abopt_heads_frag_floats': (c_size_t, []),
    'abopt_mixer_frag_floats': (c_size_t, []),
    'abopt_mlp_frag_floats': (c_size_t, []),
    'abopt_out_terms_floats': (c_size_t, []),
    'abopt_out_frag_terms': (c_int, [c_f, c_f, c_stream]),
    'abopt_pack_tail_weights': (c_int, [c_f] * 7 + [c_stream]),
    'abopt_block_tail_forward': (c_int, [c_f] * 5 + [c_u8] + [c_f] * 9 + [c_int64, c_stream]),
    'abopt_block_tail_backward': (c_int, [c_f, c_f, c_f, c_u8] + [c_f] * 6 + [c_int64, c_stream]),
    'abopt_ga_workspace_bytes': (c_size_t, [c_int] * 4),
    'abopt_ga_block_forward': (c_int, [POINTER(GaWeights)] + [c_f] * 4 + [c_u8, c_f] + [c_int] * 4 + [POINTER(GaDebug), c_void_p, c_size_t, c_stream]),
    'abopt_ga_block_forward_cached': (c_int, [POINTER(GaWeights)] + [c_f] * 4 + [c_u8, c_f] + [c_int] * 4 + [c_f, c_f, c_int, c_f, c_void_p, c_size_t, c_stream]),
    'abopt_ga_encoder_forward': (c_int, [POINTER(GaWeights), c_int] + [c_f] * 4 + [c_u8, c_f] + [c_int] * 4 + [c_void_p, c_size_t, c_stream]),
    'abopt_eps_workspace_bytes': (c_size_t, [c_int] * 4),
    'abopt_pair_bias_cache_bytes': (c_size_t, [c_int, c_int, c_int]),
    'abopt_pair_bias_cache': (c_int, [POINTER(GaWeights), c_int, c_f, c_f, c_int, c_int, c_int, c_stream]),
    'abopt_nonfinite_flag': (c_int, [c_int, c_stream]),
    'abopt_nonfinite_flag_reset': (c_int, [c_stream]),
    'abopt_pair_terms_bytes': (c_size_t, [c_int, c_int]),
    'abopt_pair_terms': (c_int, [c_f, c_f, c_int, c_int, c_int, c_stream]),
    'abopt_pair_terms_used': (c_int, [c_int, c_int, c_int]),
    'abopt_eps_net_forward': (c_int, [POINTER(EpsWeights), c_f, c_f, c_i64, c_f, c_f, c_f, c_u8, c_u8] + [c_f] * 5 + [c_int] * 5 +
                              [c_f, c_int, c_f, c_void_p, c_size_t, c_stream]),
    'abopt_denoise_step': (c_int, [POINTER(StepParams), POINTER(StepNoise), c_uint64, c_uint64, c_f, c_f, c_i64] + [c_f] * 4 + [c_u8, c_f, c_f, c_int, c_int] +
                           [c_f, c_f, c_i64] + [c_f] * 4 + [c_void_p, c_i32, c_int, c_int, c_stream]),
    'abopt_query_row_list': (c_int, [c_u8, c_int, c_int, c_void_p, c_void_p, c_stream]),
    'abopt_eps_net_step': (c_int, [POINTER(EpsWeights), c_f, c_f, c_i64, c_f, c_f, c_f, c_u8, c_u8] + [c_f] * 5 + [c_int] * 4 + [c_f, c_int, c_f, c_void_p, c_size_t] +
                           [POINTER(StepParams), POINTER(StepNoise), c_uint64, c_uint64, c_f, c_f, c_f, c_int, c_int] + [c_f, c_f, c_i64] + [c_f] * 4 +
                           [c_void_p, c_i32, c_int, c_int, c_int, c_i32, c_i32, c_int, c_stream]),
    'abopt_igso3_tables': (c_int, [c_f, c_int, c_int, c_int, c_f, c_f, c_f, c_stream]),
    'abopt_sample_init': (c_int, [c_f, c_f, c_i64, c_u8, c_f, c_f, c_i64, c_uint64, c_uint64, c_float, c_void_p, c_int, c_int, c_f, c_f, c_i64, c_i32, c_int, c_int, c_stream]),
    'abopt_add_noise': (c_int, [c_i64, c_f, c_f, c_u8, c_f, c_f, c_int, c_int, POINTER(AddNoiseNoise), c_uint64, c_uint64, c_f, c_f, c_i64, c_u8, c_float, c_void_p, c_int, c_int, c_int,
                        c_f, c_f, c_i64, c_f, c_f, c_void_p, c_i32, c_int, c_int, c_stream]),
    'abopt_dockq_workspace_bytes': (c_size_t, [c_int]),
    'abopt_dockq_lite': (c_int, [c_f, c_u8, c_int, c_f, c_u8, c_i32, c_int, c_int, c_int, c_f, c_void_p, c_size_t, c_stream]),
    'abopt_dockq_grouped_workspace_bytes': (c_size_t, [c_int, c_int]),
    'abopt_dockq_lite_grouped': (c_int, [c_f, c_u8, c_int, c_f, c_u8, c_i32] + [c_int] * 4 + [c_f, c_void_p, c_size_t, c_stream]),
    'abopt_ipa_train_workspace_bytes': (c_size_t, [c_int, c_int]),
    'abopt_ipa_core_train_forward': (c_int, [c_f] * 4 + [c_u8] + [c_f] * 5 + [c_int, c_int, c_int, c_void_p, c_size_t, c_stream]),
    'abopt_ipa_points_backward': (c_int, [c_f, c_int] + [c_f] * 5 + [c_int, c_int, c_stream]),
    'abopt_ipa_backward_operands': (c_int, [c_f] * 6 + [c_int, c_int, c_stream]),
    'abopt_ipa_backward_assemble': (c_int, [c_f] * 9 + [c_int, c_int, c_stream]),
    'abopt_ipa_pair_backward': (c_int, [c_f] * 5 + [c_int] + [c_f] * 4 + [c_int] * 4 + [c_stream]),
    'abopt_ipa_dz_assemble': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_f, c_int, c_int, c_int, c_stream]),
    'abopt_residue_embed_workspace_bytes': (c_size_t, [c_int] * 4),
    'abopt_residue_embed_forward': (c_int, [POINTER(EncodeInputs), POINTER(ResidueEmbedWeights), c_f, c_f, c_f, c_void_p, c_size_t, c_stream]),
    'abopt_residue_features_workspace_bytes': (c_size_t, [c_int, c_int]),
    'abopt_residue_features': (c_int, [POINTER(EncodeInputs), POINTER(ResidueEmbedWeights), c_f, c_f, c_f, c_void_p, c_size_t, c_stream]),
    'abopt_pair_embed_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'abopt_pair_embed_forward': (c_int, [POINTER(EncodeInputs), POINTER(PairEmbedWeights)] + [c_f] * 4 + [c_void_p, c_size_t, c_stream]),
    'abopt_pair_embed_backward_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'abopt_pair_embed_backward': (c_int, [POINTER(EncodeInputs), POINTER(PairEmbedWeights)] + [c_f] * 6 + [c_void_p, c_size_t, c_stream]),
    'abopt_dpm_losses': (c_int, [c_f] * 5 + [c_i64, c_i64, c_f, c_u8, c_int, c_int] + [c_f] * 4 + [c_stream]),
    'abopt_abdock_losses_max_length': (c_int, []),
    'abopt_abdock_losses': (c_int, [c_f] * 5 + [c_u8, c_u8, c_f, c_int, c_int, c_int, c_float, c_int, c_f, c_f, c_f, c_stream]),
    'abopt_layer_norm_forward': (c_int, [c_f, c_f, c_f, c_int, c_float, c_int64, c_f, c_f, c_f, c_stream]),
    'abopt_layer_norm_backward': (c_int, [c_f] * 4 + [c_int, c_int64, c_f, c_f, c_stream]),
    'abopt_heads_epilogue_forward': (c_int, [c_f] * 4 + [c_u8, c_f, c_f, c_f, c_int64, c_int, c_stream]),
    'abopt_heads_epilogue_backward': (c_int, [c_f, c_f, c_u8] + [c_f] * 4 + [c_int64, c_stream]),
    'abopt_reconstruct_backbone_partially': (c_int, [c_f, c_f, c_f, c_i64, c_i64, c_i64, c_u8, c_u8, c_f, c_f, c_f, c_u8, c_int, c_int, c_int, c_stream]),
    'abopt_gemm': (c_int, [c_f, c_int, c_int64, c_int, c_f, c_int, c_int64, c_int, c_f, c_int, c_int64] + [c_int] * 4 + [c_float, c_f, c_int, c_void_p, c_size_t, c_stream]),
    'abopt_gemm_tn_grouped': (c_int, [POINTER(GemmTnProblem), c_int, c_void_p, c_size_t, c_stream]),
    'abopt_colsum': (c_int, [c_f, c_int, c_int64, c_int, c_f, c_void_p, c_size_t, c_stream]),
    'abopt_bucket_colsum': (c_int, [c_f, c_int, c_int64, c_int, c_i32, c_int, c_f, c_void_p, c_size_t, c_stream]),
    'abopt_segment_bucket_colsum': (c_int, [c_f] + [c_int] * 4 + [c_i32, c_int, c_int, c_f, c_stream]),
    'abopt_adam_ws_floats': (c_size_t, [c_int, c_void_p]),
    'abopt_adam_step': (c_int, [c_int] + [c_void_p] * 5 + [c_double] * 6 + [c_i64, c_f, c_size_t, c_f, c_void_p, c_stream]),
    'abopt_commonness_score': (c_int, [c_f, c_f, c_int, c_int, c_stream]),
    'abopt_commonness_score_grouped': (c_int, [c_f, c_f, c_int, c_int, c_int, c_stream]),
    'abopt_cluster_ws_bytes': (c_size_t, [c_int, c_int]),
    'abopt_cluster_poses_grouped': (c_int, [c_f, c_int, c_int, c_int, c_float, c_int, c_void_p, c_size_t] + [c_void_p] * 4 + [c_f, c_stream]),
    'abopt_cluster_sequences_grouped': (c_int, [c_u8, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t] + [c_void_p] * 5 + [c_stream]),
    'abopt_sequence_profile_grouped': (c_int, [c_u8, c_int, c_int, c_int, c_void_p, c_stream]),
    'abopt_cluster_shapes_grouped': (c_int, [c_f, c_int, c_int, c_int, c_float, c_int, c_void_p, c_size_t] + [c_void_p] * 4 + [c_f, c_stream]),
    'abopt_interface_geometry_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'abopt_interface_geometry_grouped': (c_int, [c_f, c_u8, c_int, c_i32, c_u8] + [c_int] * 4 + [c_float] * 3 + [c_void_p] * 3 + [c_size_t, c_stream]),
    'abopt_lddt_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'abopt_lddt_ca_grouped': (c_int, [c_f, c_u8, c_int, c_f, c_u8, c_u8, c_i32] + [c_int] * 4 + [c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_stream]),
    'abopt_lddt_ca_ensemble': (c_int, [c_f, c_u8, c_int, c_u8, c_i32] + [c_int] * 4 + [c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_stream]),
    'abopt_sasa_ws_bytes': (c_size_t, [c_int] * 4),
    'abopt_sasa_grouped': (c_int, [c_f, c_u8, c_int, c_i32, c_f, c_f] + [c_int] * 5 + [c_float] * 2 + [c_void_p] * 3 + [c_size_t, c_stream]),
    'abopt_guide_positions': (c_int, [c_f, c_f, c_u8, c_u8, c_i32, c_int, c_int, c_int] + [c_float] * 6 + [c_void_p, c_stream]),
    'abopt_relax_max_moved': (c_int, []),
    'abopt_relax_grouped': (c_int, [c_f, c_f, c_u8, c_int, c_u8, c_u8] + [c_int] * 5 + [c_float] * 8 + [c_int, c_f, c_stream]),
    'abopt_sequence_liabilities_grouped': (c_int, [c_u8, c_u8, c_u8] + [c_int] * 4 + [c_void_p] * 3 + [c_stream]),
    'abopt_surface_patches_grouped': (c_int, [c_f, c_u8, c_int, c_i32, c_f, c_u8, c_int, c_f, c_float] + [c_int] * 4 + [c_void_p, c_void_p, c_stream]),
    'abopt_interface_energy_grouped': (c_int, [c_f, c_u8, c_int, c_i32, c_u8, c_int, c_u8, c_f, c_f] + [c_int] * 4 + [c_float] * 6 + [c_void_p, c_void_p, c_stream]),
    'abopt_backbone_max_rows': (c_int, []),
    'abopt_backbone_conformation_grouped': (c_int, [c_f, c_u8, c_int, c_u8, c_u8, c_int, c_u8, c_f] + [c_int] * 5 + [c_float] + [c_void_p] * 8 + [c_stream]),
    'abopt_align_sequences': (c_int, [c_u8, c_u8, c_u8, c_u8, c_i32] + [c_int] * 7 + [c_void_p] * 3 + [c_stream]),
    'abopt_gapped_rmsd': (c_int, [c_f, c_u8, c_f, c_u8] + [c_int] * 4 + [c_void_p, c_void_p, c_stream]),
    'abopt_superposed_rmsd': (c_int, [c_f, c_u8, c_u8, c_f, c_u8, c_u8] + [c_int] * 4 + [c_void_p] * 5 + [c_stream]),
    'abopt_align_traceback': (c_int, [c_u8, c_u8, c_u8, c_u8, c_i32] + [c_int] * 3 + [c_i32] + [c_int] * 5 + [c_void_p] * 6 + [c_stream]),
    'abopt_superposed_rmsd_mapped': (c_int, [c_f, c_f, c_void_p, c_i32, c_int] + [c_u8] * 4 + [c_int] * 4 + [c_void_p] * 5 + [c_stream]),
    'abopt_prof_enable': (c_int, [c_int]),
    'abopt_prof_spans_reset': (c_int, [c_stream]),
    'abopt_prof_spans': (c_int, [POINTER(c_int), POINTER(c_double)]),
    'abopt_prof_collect': (c_int, [POINTER(c_int), POINTER(c_double)]),
    'abopt_prof_clock': (c_int, [POINTER(c_longlong), POINTER(c_longlong)]),
    'abopt_prof_peek': (c_int, [POINTER(c_int), POINTER(c_double)]),
}
EXPORTS = list(_SIGNATURES)

_lib = None
_lock = threading.Lock()


def lib():
    """Load the shared library once; raise (never fall back) if it is absent or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                               '(or `make -C ab_opt_amd/csrc`).  ab_opt_amd has no non-HIP execution path.')
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(L, name)     # AttributeError here = a symbol of include/abopt.h is missing
            fn.restype, fn.argtypes = restype, argtypes
        if L.abopt_abi_version() != ABI_VERSION:
            raise RuntimeError(f'libabopt_hip.so ABI {L.abopt_abi_version()} != expected {ABI_VERSION}; rebuild it')
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError(f'abopt error {rc}: {lib().abopt_last_error().decode()}')


_DT = {torch.float32: 'f32', torch.int64: 'i64', torch.bool: 'u8', torch.uint8: 'u8'}


def ptr(t, dtype=None, optional=False, strided=False):
    """Device pointer of a contiguous HIP tensor (None -> NULL when optional).  strided=True: the caller passes the strides itself."""
    if t is None:
        if optional:
            return None
        raise ValueError('required tensor is None')
    if not t.is_cuda:
        raise RuntimeError('ab_opt_amd kernels run on a HIP device only; got a CPU tensor (there is no CPU path)')
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        raise RuntimeError(f'tensor lives on {t.device} but the current HIP device is cuda:{torch.cuda.current_device()}: kernels launch on '
                           'the current device/stream -- call torch.cuda.set_device() (one process per GPU) or wrap the call in '
                           '`with torch.cuda.device(tensor.device):`')
    if not strided and not t.is_contiguous():
        raise ValueError('tensor must be contiguous')
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f'expected {dtype}, got {t.dtype}')
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _contig(*ts):
    """Contiguous versions of the arguments, returned as objects the CALLER binds to locals: a temporary
    `x.contiguous()` inside an argument list is freed as soon as its address is taken, and the caching allocator hands
    the same block to the next temporary -- two kernel arguments would then alias."""
    return [t if (t is None or t.is_contiguous()) else t.contiguous() for t in ts]


class Workspace:
    """Grow-only scratch buffer per (device, stream)."""
    _bufs = {}

    @classmethod
    def get(cls, nbytes, device):
        key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
        buf = cls._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            cls._bufs[key] = buf
        return buf

    @classmethod
    @contextlib.contextmanager
    def private(cls):
        """`with Workspace.private() as keep:` around a stream capture.  Inside, no buffer from before is visible, so every buffer the recorded launches use is
        allocated inside the capture, from the graph's own pool; on exit those buffers are in the list `keep` -- whoever holds the graph holds it, for as long --
        and the buffers from before are back, untouched.
        Why hiding and not only "keep the keys that are new": torch records every capture on ONE stream (torch.cuda.graph.default_capture_stream), so the key of
        that stream is usually there already, left by an earlier capture, and its buffer lives in that earlier graph's pool.  A capture that finds it large
        enough records launches that point into a foreign pool; one that finds it too small replaces it, the replacement is then nobody's, and the next
        capture that needs more drops it in turn.  Either way a live graph ends up pointing at a freed block of a pool whose graph is gone, and
        torch.cuda.graph.__enter__ calls torch.cuda.empty_cache(), which gives the free blocks of such pools back to the device: the next replay of that graph
        then writes into memory that is unmapped or somebody else's."""
        held = dict(cls._bufs)
        cls._bufs.clear()
        keep = []
        try:
            yield keep
        finally:
            keep.extend(cls._bufs.values())
            cls._bufs.clear()
            cls._bufs.update(held)


def device_info():
    cu, lds = C.c_int(), C.c_int()
    arch = C.create_string_buffer(64)
    _check(lib().abopt_device_info(C.byref(cu), C.byref(lds), arch, 64))
    return dict(cu_count=cu.value, lds_bytes_per_cu=lds.value, arch=arch.value.decode())


# ------------------------------------------------------------------------------- thin wrappers
def so3_exp(w):
    w = w.contiguous()
    R = torch.empty(w.shape[:-1] + (3, 3), dtype=torch.float32, device=w.device)
    _check(lib().abopt_so3_exp(ptr(w, torch.float32), ptr(R), w.numel() // 3, stream()))
    return R


def so3_log(R, grad_mode=False):
    R = R.contiguous()
    w = torch.empty(R.shape[:-2] + (3,), dtype=torch.float32, device=R.device)
    _check(lib().abopt_so3_log(ptr(R, torch.float32), ptr(w), R.numel() // 9, int(grad_mode), stream()))
    return w


def ga_weights_struct(t):
    """t: dict name -> contiguous device tensor with the field names of GaWeights (w_node_frag optional)."""
    s = GaWeights()
    for name, _ in GaWeights._fields_:
        setattr(s, name, ptr(t.get(name), torch.float32, optional=name in ('w_node_frag', 'w_out_frag', 'w_mlp_frag', 'w_out_terms')))
    return s


def pack_mfma_operand(w):
    """w [32 B, K] (K a multiple of 16) -> [B, K/16, 2, 64, 4] flattened + {S, 1 / S, 0, 0}: 32x32x16 MFMA operand order, every weight as the two
    fp16 terms of S w (fp32 container of 8 fp16 per lane), S = tail_weight_scale(w):
    [cb][step][term][lane = 32 khalf + c][i] = term(S w[32 cb + c][16 step + 8 khalf + i])."""
    R, K = w.shape
    S = tail_weight_scale(w)
    g = w.float() * S
    h16 = g.half()
    terms = torch.stack([h16, (g - h16.float()).half()], 0)   # [term, R, K] fp16
    g = terms.reshape(2, R // 32, 32, K // 16, 2, 8)          # [term, cb, col, step, k half, i]
    out = g.permute(1, 3, 0, 4, 2, 5).contiguous()            # [cb, step, term, k half, col, i]
    return torch.cat([out.view(-1).view(torch.float32), torch.tensor([S, 1.0 / S, 0.0, 0.0], dtype=torch.float32, device=w.device)])


def pack_heads_weights(w_head1, w_crd2, w_rot2, w_seq2, w_crd3, w_rot3, w_seq3):
    """-> w_heads_frag [27, 8, 2, 64, 4] + {S, 1 / S, 0, 0} (include/abopt.h: abopt_eps_weights.w_heads_frag)."""
    pad32 = lambda w: torch.cat([w, torch.zeros(32 - w.shape[0], w.shape[1], dtype=w.dtype, device=w.device)], 0)
    rows = torch.cat([w_head1[:, :128], w_crd2, w_rot2, w_seq2, pad32(w_crd3), pad32(w_rot3), pad32(w_seq3)], 0)      # [27 * 32, 128]
    return pack_mfma_operand(rows.contiguous())


def out_feat_order():
    """The order in which the 1824 feature columns enter the tail's K index (csrc/tail_common.h: ot_feat_col): the 768 pair-feature columns
    (head h, channel ch) sit at K index 192 * ((ch % 16) // 4) + 16 h + 4 (ch // 16) + ch % 4, the other columns keep their place."""
    k = torch.arange(1824)
    c, j = k // 192, k % 192
    perm = (j >> 4) * 64 + ((j >> 2) & 3) * 16 + 4 * c + (j & 3)
    return torch.where(k < 768, perm, k)


def tail_weight_scale(w):
    """Power of two S with max |w| S in [2^14, 2^15) (csrc/mlp.hip: tail_weight_absmax_kernel): the weights of the forward tail are split into two
    fp16 terms of S w, so that the low terms stay normal; 1 for an all-zero matrix."""
    a = w.detach().float().abs()
    m = float(a[torch.isfinite(a)].max()) if bool(torch.isfinite(a).any()) else 0.0
    if m <= 0.0:
        return 1.0
    import math
    e = 15 - math.frexp(m)[1]
    return math.ldexp(1.0, max(-100, min(100, e)))


def _fp16_terms(v):
    """[..., 8] fp32 -> (h, l) as [..., 4] fp32 words holding 8 fp16 each: h = fp16(v), l = fp16(v - h), round to nearest (csrc/ipa_common.h: split_pair2)."""
    h = v.half()
    lo = (v - h.float()).half()
    return h.contiguous().view(torch.float32), lo.contiguous().view(torch.float32)


def pack_out_weights(w_out):
    """w_out [128, 1824] -> w_out_frag [4 cb, 114 k-steps, 2 terms, 64 lanes, 8 fp16] (as 128 * 1824 fp32 words) in 32x32x16 operand order
    (include/abopt.h: abopt_ga_weights.w_out_frag): lane 32 kh + c holds the two fp16 terms of S w_out[32 cb + c][col(16 s + 8 kh + i)]."""
    w = w_out.float()[:, out_feat_order().to(w_out.device)] * tail_weight_scale(w_out)
    v = w.reshape(4, 32, 114, 2, 8).permute(0, 2, 3, 1, 4).reshape(4, 114, 64, 8)           # [cb, s, lane = 32 kh + c, i]
    h, lo = _fp16_terms(v)
    return torch.stack([h, lo], dim=2).contiguous()                                              # [cb, s, term, lane, 4 words]


def pack_mlp_weights(w0, w1, w2):
    """three [128, 128] layers -> w_mlp_frag (include/abopt.h: abopt_ga_weights.w_mlp_frag): [layer][ct][s][term][lane = 16 kq + m] x 8 fp16 =
    the two fp16 terms of S_layer w[16 ct + m][32 s + 8 kq + i], then {S_out = 0 here, S_0, S_1, S_2, 1 / S ...} -- the caller of the device packer
    gets S_out filled in; this host statement takes it from `pack_mlp_weights.s_out` when set -- zero-padded to abopt_mlp_frag_floats() floats."""
    out, scales = [], []
    for w in (w0, w1, w2):
        S = tail_weight_scale(w)
        scales.append(S)
        v = (w.float() * S).reshape(8, 16, 4, 4, 8).permute(0, 2, 3, 1, 4).reshape(8, 4, 64, 8)   # [ct, m, s, kq, i] -> [ct, s, lane = 16 kq + m, i]
        h, lo = _fp16_terms(v)
        out.append(torch.stack([h, lo], dim=2).reshape(-1))
    flat = torch.cat(out)
    return flat, scales


def pack_tail_weights_host(w_out, w0, w1, w2):
    """Host statement of abopt_pack_tail_weights' forward buffers: (w_out_frag, w_mlp_frag), bit for bit what the device packer writes."""
    wof = pack_out_weights(w_out).flatten()
    flat, scales = pack_mlp_weights(w0, w1, w2)
    S = [tail_weight_scale(w_out)] + scales
    sc = torch.tensor(S + [1.0 / v for v in S], dtype=torch.float32, device=flat.device)
    pad = torch.zeros(lib().abopt_mlp_frag_floats() - flat.numel() - 8, dtype=torch.float32, device=flat.device)
    return wof, torch.cat([flat, sc, pad])


_NODE_FRAG_INDEX = None

def split_bf16x3(w):
    """fp32 tensor -> (h, m, l) int16 bf16 bit patterns with h + m + l == w exactly (csrc/node_frags.hip: split3): each term is the
    round-to-nearest bf16 of what the previous terms left."""
    def rne(v):
        return v.to(torch.bfloat16).to(torch.float32)
    h = rne(w)
    r1 = w - h
    m = rne(r1)
    l = rne(r1 - m)
    return [(v.contiguous().view(torch.int32) >> 16).to(torch.int16) for v in (h, m, l)]


def pack_node_weights(w_node):
    """w_node [2016, 128] -> w_node_frag [12 heads, 12 tiles, 4 k-steps, 2 fp16 terms, 64 lanes, 4] (fp32 container of 8 fp16 per lane) +
    {S, 1 / S, 0, 0} (include/abopt.h: abopt_node_frag_source_row): the per-head, tile-ordered, operand-order copy the fused projection kernel keeps
    in LDS, every weight as h = fp16(S w), l = fp16(S w - h) with S = tail_weight_scale(w_node).  Index tables come from the library so the layout
    has one owner."""
    global _NODE_FRAG_INDEX
    if _NODE_FRAG_INDEX is None:
        L_ = lib()
        rows = torch.tensor([[[L_.abopt_node_frag_source_row(h, T, m) for m in range(16)] for T in range(12)] for h in range(12)], dtype=torch.long)
        _NODE_FRAG_INDEX = rows
    rows = _NODE_FRAG_INDEX.to(w_node.device)
    S = tail_weight_scale(w_node)
    wz = torch.cat([w_node, torch.zeros(1, w_node.shape[1], dtype=w_node.dtype, device=w_node.device)], 0)
    g = wz[torch.where(rows >= 0, rows, torch.full_like(rows, w_node.shape[0]))].float() * S   # [12, 12, 16 (m), 128]
    h16 = g.half()
    terms = torch.stack([h16, (g - h16.float()).half()], 0)                                # [2, h, T, m, 128] fp16
    terms = terms.reshape(2, 12, 12, 16, 4, 4, 8)                                          # [term, h, T, m, s, kq, i]: k = 32 s + 8 kq + i
    out = terms.permute(1, 2, 4, 0, 5, 3, 6).contiguous()                                  # [h, T, s, term, kq, m, i] == [h][T][s][term][lane = 16 kq + m][i]
    return torch.cat([out.view(-1).view(torch.float32), torch.tensor([S, 1.0 / S, 0.0, 0.0], dtype=torch.float32, device=w_node.device)])


def ga_block_forward(ws, R, t, x, z, mask, debug=False):
    N, L, F = x.shape
    Cd = z.shape[-1]
    out = torch.empty_like(x)
    dbg, extras = None, {}
    if debug:
        extras = dict(logits=torch.empty(N, L, L, 12, device=x.device), alpha=torch.empty(N, L, L, 12, device=x.device),
                      feat=torch.empty(N, L, 1824, device=x.device))
        dbg = GaDebug(ptr(extras['logits']), ptr(extras['alpha']), ptr(extras['feat']))
    nb = lib().abopt_ga_workspace_bytes(N, L, F, Cd)
    buf = Workspace.get(nb, x.device)
    R, t, x, z, mask = _contig(R, t, x, z, mask)      # copies (if any) stay alive until the launch is enqueued
    _check(lib().abopt_ga_block_forward(C.byref(ws), ptr(R, torch.float32), ptr(t, torch.float32), ptr(x, torch.float32), ptr(z, torch.float32),
                                        ptr(mask, torch.bool), ptr(out), N, L, F, Cd,
                                        C.byref(dbg) if dbg is not None else None, ptr(buf), buf.numel(), stream()))
    return (out, extras) if debug else out


def ga_block_forward_cached(ws, R, t, x, z, mask, pair_bias_cache, pair_terms=None, pair_feat_shared=0, want_feat=False):
    """One block with this block's slice of the bias cache and (optionally) the pair terms (include/abopt.h: abopt_ga_block_forward_cached)."""
    N, L, F = x.shape
    Cd = z.shape[-1]
    out = torch.empty_like(x)
    feat = torch.empty(N, L, 1824, device=x.device) if want_feat else None
    nb = lib().abopt_ga_workspace_bytes(N, L, F, Cd)
    buf = Workspace.get(nb, x.device)
    R, t, x, z, mask = _contig(R, t, x, z, mask)
    _check(lib().abopt_ga_block_forward_cached(C.byref(ws), ptr(R, torch.float32), ptr(t, torch.float32), ptr(x, torch.float32), ptr(z, torch.float32),
                                               ptr(mask, torch.bool), ptr(out), N, L, F, Cd, ptr(pair_bias_cache, torch.float32),
                                               ptr(pair_terms, torch.float32, optional=True), int(pair_feat_shared), ptr(feat, optional=True),
                                               ptr(buf), buf.numel(), stream()))
    return (out, feat) if want_feat else out


def ga_encoder_forward(ws_array, num_layers, R, t, x, z, mask):
    N, L, F = x.shape
    Cd = z.shape[-1]
    out = torch.empty_like(x)
    nb = lib().abopt_ga_workspace_bytes(N, L, F, Cd)
    buf = Workspace.get(nb, x.device)
    R, t, x, z, mask = _contig(R, t, x, z, mask)
    _check(lib().abopt_ga_encoder_forward(ws_array, num_layers, ptr(R, torch.float32), ptr(t, torch.float32), ptr(x, torch.float32),
                                          ptr(z, torch.float32), ptr(mask, torch.bool), ptr(out), N, L, F, Cd, ptr(buf), buf.numel(), stream()))
    return out


def eps_net_forward(ew, v_t, p_t, s_t, res_feat, pair_feat, beta, mask_generate, mask_res, has_prmsd, num_bins, grad_mode=False, out=None,
                    pair_bias_cache=None, pair_feat_shared=False, pair_terms=None):
    N, L = mask_res.shape
    F, Cd = res_feat.shape[-1], pair_feat.shape[-1]
    dev = res_feat.device
    if out is None:
        out = dict(v_next=torch.empty(N, L, 3, device=dev), R_next=torch.empty(N, L, 3, 3, device=dev),
                   eps_pos=torch.empty(N, L, 3, device=dev), c=torch.empty(N, L, 20, device=dev),
                   prmsd_logits=torch.empty(N, num_bins, device=dev) if has_prmsd else None)
    nb = lib().abopt_eps_workspace_bytes(N, L, F, Cd)
    buf = Workspace.get(nb, dev)
    v_t, p_t, s_t, res_feat, pair_feat, beta, mask_generate, mask_res = _contig(v_t, p_t, s_t, res_feat, pair_feat, beta, mask_generate, mask_res)
    _check(lib().abopt_eps_net_forward(C.byref(ew), ptr(v_t, torch.float32), ptr(p_t, torch.float32), ptr(s_t, torch.int64), ptr(res_feat, torch.float32),
                                       ptr(pair_feat, torch.float32), ptr(beta, torch.float32), ptr(mask_generate, torch.bool), ptr(mask_res, torch.bool),
                                       ptr(out['v_next']), ptr(out['R_next']), ptr(out['eps_pos']), ptr(out['c']),
                                       ptr(out['prmsd_logits'], optional=True), N, L, F, Cd, int(grad_mode),
                                       ptr(pair_bias_cache, torch.float32, optional=True), int(pair_feat_shared),
                                       ptr(pair_terms, torch.float32, optional=True), ptr(buf), buf.numel(), stream()))
    return out


def pair_bias_cache_bytes(N, L, num_layers):
    return lib().abopt_pair_bias_cache_bytes(N, L, num_layers)


def nonfinite_flag(reset=True):
    """Synchronises the current stream and returns whether any eps_net_forward since the last reset produced a non-finite head output
    (include/abopt.h: abopt_nonfinite_flag -- the range guard of the two-term fp16 layers)."""
    r = lib().abopt_nonfinite_flag(int(reset), stream())
    if r < 0:
        raise RuntimeError('abopt_nonfinite_flag: ' + last_error())
    return bool(r)


def nonfinite_flag_reset():
    """Clears the flag in stream order on the current stream: no synchronisation (include/abopt.h: abopt_nonfinite_flag_reset)."""
    _check(lib().abopt_nonfinite_flag_reset(stream()))


def pair_terms_bytes(N, L):
    return lib().abopt_pair_terms_bytes(N, L)


def pair_terms_used(N, L, pair_feat_shared=0):
    """Whether eps_net_forward(N, L) with a bias cache takes the kernels that read pair terms on this device (include/abopt.h: abopt_pair_terms_used)."""
    return bool(lib().abopt_pair_terms_used(N, L, int(pair_feat_shared)))


def pair_terms(pair_feat):
    """pair_feat as K-packed two-term fp16 operands of the pair aggregation + one power-of-two scale per query row, once per sampling call
    (include/abopt.h: abopt_pair_terms).  Returns the blob eps_net_forward(pair_terms=...) takes."""
    N, L = pair_feat.shape[:2]
    blob = torch.empty(lib().abopt_pair_terms_bytes(N, L) // 4, dtype=torch.float32, device=pair_feat.device)
    pair_feat, = _contig(pair_feat)
    _check(lib().abopt_pair_terms(ptr(pair_feat, torch.float32), ptr(blob), N, L, pair_feat.shape[-1], stream()))
    return blob


def pair_bias_cache(blocks_array, num_layers, pair_feat):
    """proj_pair_bias(pair_feat) of every block, once per sampling call (include/abopt.h: abopt_pair_bias_cache)."""
    N, L = pair_feat.shape[:2]
    nb = lib().abopt_pair_bias_cache_bytes(N, L, num_layers)
    cache = torch.empty(nb // 4, dtype=torch.float32, device=pair_feat.device)
    pair_feat, = _contig(pair_feat)
    _check(lib().abopt_pair_bias_cache(blocks_array, num_layers, ptr(pair_feat, torch.float32), ptr(cache), N, L,
                                       pair_feat.shape[-1], stream()))
    return cache


def query_row_list(mask_generate):
    """mask_generate (N, L) -> (rows, count): per sample the ascending indices of its generated residues, -1 behind them (int32, (N, ceil(L / 16) * 16)), and their
    number (int32, (N,)) -- one launch, nothing read on the host (include/abopt.h: abopt_query_row_list).  With tiles = ceil(count.max() / 16) the triple
    (rows, count, tiles) is what eps_net_step(query_rows=...) takes."""
    N, L = mask_generate.shape
    mask_generate, = _contig(mask_generate)
    rows = torch.empty(N, (L + 15) // 16 * 16, dtype=torch.int32, device=mask_generate.device)
    count = torch.empty(N, dtype=torch.int32, device=mask_generate.device)
    _check(lib().abopt_query_row_list(ptr(mask_generate, torch.bool), N, L, ptr(rows), ptr(count), stream()))
    return rows, count


def check_temperature(name, tau):
    """float(tau) of a sampling temperature (include/abopt.h: seq_temperature), or ValueError: it must be finite and >= 0, and a non-zero one below 1e-3 is refused
    -- the kernel multiplies by 1 / tau in fp32; 0 is the greedy limit and has a path of its own.  No device is needed."""
    import math
    t = float(tau)
    if not math.isfinite(t) or t < 0.0:
        raise ValueError(f'{name} must be finite and >= 0 (got {tau!r})')
    if 0.0 < t < 1e-3:
        raise ValueError(f'{name} must be 0 (greedy) or at least 1e-3 (got {tau!r})')
    return t


def check_noise_scale(name, lam):
    """float(lam) of a structure-noise scale (include/abopt.h: noise_scale), or ValueError for a negative or non-finite one.  No device is needed."""
    import math
    s = float(lam)
    if not math.isfinite(s) or s < 0.0:
        raise ValueError(f'{name} must be finite and >= 0 (got {lam!r})')
    return s


GUIDE_DECAY = {'constant': 0, 'linear': 1, 'quadratic': 2}      # guide_decay -> k of the step weight g(u) = (u / num_steps)^k


def check_guidance(guide_attract=0.0, guide_attract_radius=8.0, guide_repel=0.0, guide_repel_radius=3.0, guide_max_shift=2.0, guide_decay='constant'):
    """The knobs of guided sampling (include/abopt.h: abopt_guide_positions) as a dict of floats under their own names plus guide_decay as
    its exponent k (0, 1, 2; the names of GUIDE_DECAY, or k itself), or ValueError: every scalar finite and >= 0, guide_attract <= 1 (the pull may not overshoot),
    guide_max_shift > 0.  No device is needed.  8, 3 and 2 Angstrom are conventional values, not tuned ones."""
    import math
    out = {}
    for name, v in (('guide_attract', guide_attract), ('guide_attract_radius', guide_attract_radius), ('guide_repel', guide_repel),
                    ('guide_repel_radius', guide_repel_radius), ('guide_max_shift', guide_max_shift)):
        f = float(v)
        if not math.isfinite(f) or f < 0.0:
            raise ValueError(f'{name} must be finite and >= 0 (got {v!r})')
        out[name] = f
    if out['guide_attract'] > 1.0:
        raise ValueError(f'guide_attract must be <= 1: a larger weight would pull the generated residues past the hotspots (got {guide_attract!r})')
    if out['guide_max_shift'] == 0.0:
        raise ValueError('guide_max_shift must be > 0')
    if isinstance(guide_decay, str):
        if guide_decay not in GUIDE_DECAY:
            raise ValueError(f'guide_decay must be one of {sorted(GUIDE_DECAY)} (got {guide_decay!r})')
        out['guide_decay'] = GUIDE_DECAY[guide_decay]
    else:
        if isinstance(guide_decay, bool) or guide_decay not in (0, 1, 2):
            raise ValueError(f'guide_decay must be one of {sorted(GUIDE_DECAY)} or their exponents 0, 1, 2 (got {guide_decay!r})')
        out['guide_decay'] = int(guide_decay)
    return out


def guide_weight(u, num_steps, decay):
    """g(u) = (u / num_steps)^k of the step that lands on u, in float64 (the caller multiplies a weight by it and rounds the product once to fp32)."""
    return (float(u) / float(num_steps)) ** int(decay) if int(decay) else 1.0


def guide_positions(p, p_norm, mask_generate, mask_res, role, w_att=0.0, r_att=8.0, w_rep=0.0, r_rep=3.0, max_shift=2.0, position_scale=10.0,
                    position_mean=(0.0, 0.0, 0.0), role_shared=0):
    """One guidance nudge, in place (include/abopt.h: abopt_guide_positions): p (N, L, 3) fp32 in Angstrom and -- optional -- p_norm, its
    normalised copy; mask_generate, mask_res (N, L) bool; role (N, L) int32, or (N / role_shared, L) shared by role_shared consecutive samples: bit 0 hotspot,
    bit 1 repeller.  Only the rows gen & res change.  Stream-ordered, no host synchronisation, capturable.  -> p."""
    ptr(p, strided=True)                                            # a CPU tensor is refused here, before anything else
    kn = check_guidance(w_att, r_att, w_rep, r_rep, max_shift)
    if p.dim() != 3 or p.shape[2] != 3 or mask_generate.shape != p.shape[:2] or mask_res.shape != p.shape[:2]:
        raise ValueError(f'guide_positions: expected p (N, L, 3) and masks (N, L), got {tuple(p.shape)}, {tuple(mask_generate.shape)} and {tuple(mask_res.shape)}')
    N, L = mask_res.shape
    S = int(role_shared)
    if S < 0 or (N % S if S else 0) or role.dim() != 2 or tuple(role.shape) != ((N // S if S else N), L):
        raise ValueError(f'guide_positions: role {tuple(role.shape)} does not fit {N} samples of {L} residues with role_shared={role_shared}')
    if p_norm is not None and p_norm.shape != p.shape:
        raise ValueError('guide_positions: p_norm must have the shape of p')
    mean = (C.c_float * 3)(*[float(m) for m in position_mean])
    _check(lib().abopt_guide_positions(ptr(p, torch.float32), ptr(p_norm, torch.float32, optional=True), ptr(mask_generate), ptr(mask_res), ptr(role, torch.int32),
                                       S, N, L, kn['guide_attract'], kn['guide_attract_radius'], kn['guide_repel'], kn['guide_repel_radius'],
                                       kn['guide_max_shift'], float(position_scale), mean, stream()))
    return p


def _allowed_ptr(aa_allowed, mask_generate):
    """aa_allowed (optional): contiguous int32 (N, L) device tensor, bit k of a word = residue type k may be drawn there (include/abopt.h)."""
    if aa_allowed is not None and aa_allowed.shape != mask_generate.shape:
        raise ValueError(f'aa_allowed must have the shape of mask_generate {tuple(mask_generate.shape)}, got {tuple(aa_allowed.shape)}')
    return ptr(aa_allowed, torch.int32, optional=True)


def denoise_step(sp, noise, seed, offset, v_t, p_t, s_t, v_net, p_net, c_net, prmsd_logits, mask_generate,
                 ig_X_row, ig_cdf_row, num_bins, out, want_post=False, seed_dev=None, aa_allowed=None):
    """seed_dev (optional): int64 device tensor {seed, offset} read by the kernel in place of the two host values (graph replays).
    aa_allowed (optional): the allowed residue types per residue (_allowed_ptr)."""
    N, L = mask_generate.shape
    nz = None
    if noise is not None:
        nz = StepNoise(ptr(noise['axis'], torch.float32), ptr(noise['bin'], torch.int64), ptr(noise['ubin'], torch.float32),
                       ptr(noise['gauss'], torch.float32), ptr(noise['z'], torch.float32), ptr(noise['s_next'], torch.int64))
    post = torch.empty(N, L, 20, device=v_t.device) if want_post else None
    _check(lib().abopt_denoise_step(C.byref(sp), C.byref(nz) if nz is not None else None, seed, offset,
                                    ptr(v_t, torch.float32), ptr(p_t, torch.float32), ptr(s_t, torch.int64),
                                    ptr(v_net, torch.float32), ptr(p_net, torch.float32), ptr(c_net, torch.float32),
                                    ptr(prmsd_logits, optional=True), ptr(mask_generate, torch.bool),
                                    ptr(ig_X_row, torch.float32), ptr(ig_cdf_row, optional=True), ig_X_row.numel(), num_bins,
                                    ptr(out['v']), ptr(out['p']), ptr(out['s']), ptr(out.get('prmsd'), optional=True),
                                    ptr(out.get('ppl'), optional=True), ptr(post, optional=True), ptr(out.get('p_norm'), optional=True),
                                    ptr(seed_dev, torch.int64, optional=True), _allowed_ptr(aa_allowed, mask_generate), N, L, stream()))
    return post


def eps_net_step(ew, v_t, p_t, s_t, res_feat, pair_feat, beta, mask_generate, mask_res, num_bins, net, sp, noise, seed, offset, p_angstrom, ig_X_row, ig_cdf_row, out,
                 pair_bias_cache=None, pair_feat_shared=False, pair_terms=None, want_post=False, seed_dev=None, aa_allowed=None, carry_in=False, carry_out=False,
                 context_outputs_unused=False, query_rows=None):
    """One loop iteration in one C call (include/abopt.h: abopt_eps_net_step): eps_net_forward(..., out=net) then denoise_step(..., out) on its outputs, bit-identical
    to the two calls; where the library fuses the step's tail, carry_out leaves the next evaluation's mixer output in the workspace and carry_in says the previous
    call did so for exactly this v_t / s_t.  net: the dict eps_net_forward fills (prmsd_logits None without the head); out: as for denoise_step.
    context_outputs_unused: the caller reads `net` on generated residues only; `out` and the posterior are what they are without it.
    query_rows (implies context_outputs_unused): (rows, count, tiles) -- query_row_list(mask_generate) of THIS mask and the number of 16-row tiles of the list its
    longest sample fills; the same results, with the last block on listed rows only where the library's plan takes that form."""
    N, L = mask_res.shape
    F, Cd = res_feat.shape[-1], pair_feat.shape[-1]
    nz = None
    if noise is not None:
        nz = StepNoise(ptr(noise['axis'], torch.float32), ptr(noise['bin'], torch.int64), ptr(noise['ubin'], torch.float32),
                       ptr(noise['gauss'], torch.float32), ptr(noise['z'], torch.float32), ptr(noise['s_next'], torch.int64))
    post = torch.empty(N, L, 20, device=v_t.device) if want_post else None
    buf = Workspace.get(lib().abopt_eps_workspace_bytes(N, L, F, Cd), res_feat.device)
    v_t, p_t, s_t, res_feat, pair_feat, beta, mask_generate, mask_res = _contig(v_t, p_t, s_t, res_feat, pair_feat, beta, mask_generate, mask_res)
    rows, count, tiles = query_rows if query_rows is not None else (None, None, 0)
    if query_rows is not None and (rows.shape != (N, (L + 15) // 16 * 16) or count.shape != (N,)):
        raise ValueError(f'query_rows: a list of shape {tuple(rows.shape)} / {tuple(count.shape)} does not belong to a mask of shape {(N, L)}')
    _check(lib().abopt_eps_net_step(
        C.byref(ew), ptr(v_t, torch.float32), ptr(p_t, torch.float32), ptr(s_t, torch.int64), ptr(res_feat, torch.float32),
        ptr(pair_feat, torch.float32), ptr(beta, torch.float32), ptr(mask_generate, torch.bool), ptr(mask_res, torch.bool),
        ptr(net['v_next']), ptr(net['R_next']), ptr(net['eps_pos']), ptr(net['c']), ptr(net['prmsd_logits'], optional=True),
        N, L, F, Cd, ptr(pair_bias_cache, torch.float32, optional=True), int(pair_feat_shared),
        ptr(pair_terms, torch.float32, optional=True), ptr(buf), buf.numel(),
        C.byref(sp), C.byref(nz) if nz is not None else None, seed, offset, ptr(p_angstrom, torch.float32),
        ptr(ig_X_row, torch.float32), ptr(ig_cdf_row, optional=True), ig_X_row.numel(), num_bins,
        ptr(out['v']), ptr(out['p']), ptr(out['s']), ptr(out.get('prmsd'), optional=True), ptr(out.get('ppl'), optional=True),
        ptr(post, optional=True), ptr(out.get('p_norm'), optional=True), ptr(seed_dev, torch.int64, optional=True),
        _allowed_ptr(aa_allowed, mask_generate), int(carry_in), int(carry_out),
        int(bool(context_outputs_unused) or query_rows is not None), ptr(rows, torch.int32, optional=True), ptr(count, torch.int32, optional=True), int(tiles), stream()))
    return post


def igso3_tables(stddevs, bins=8192, iters=1024):
    """stddevs: fp32 device tensor (rows,) -> (X (rows, bins), Y (rows, bins), cdf (rows, bins - 1)): the IGSO(3) angle histograms of ApproxAngularDistribution for
    arbitrary standard deviations, built on the device (abopt_igso3_tables: factors and the sum over l in fp64)."""
    stddevs = stddevs.contiguous()
    rows = stddevs.numel()
    f32 = dict(dtype=torch.float32, device=stddevs.device)
    X, Y, cdf = torch.empty(rows, bins, **f32), torch.empty(rows, bins, **f32), torch.empty(rows, bins - 1, **f32)
    _check(lib().abopt_igso3_tables(ptr(stddevs, torch.float32), rows, int(bins), int(iters), ptr(X), ptr(Y), ptr(cdf), stream()))
    return X, Y, cdf


def sample_init(v, p, s, mask_generate, init_noise, seed, offset, scale, mean, sample_structure, sample_sequence, aa_allowed=None):
    N, L = mask_generate.shape
    v_i, p_i, s_i = torch.empty_like(v), torch.empty_like(p), torch.empty_like(s)
    q4 = pn = sr = None
    if init_noise is not None:
        q4, pn, sr = init_noise.get('q4'), init_noise.get('p'), init_noise.get('s')
    mean_arr = (C.c_float * 3)(*[float(m) for m in mean])
    v, p, s, mask_generate = _contig(v, p, s, mask_generate)
    _check(lib().abopt_sample_init(ptr(v, torch.float32), ptr(p, torch.float32), ptr(s, torch.int64),
                                   ptr(mask_generate, torch.bool), ptr(q4, optional=True), ptr(pn, optional=True),
                                   ptr(sr, optional=True), seed, offset, float(scale), mean_arr, int(sample_structure), int(sample_sequence),
                                   ptr(v_i), ptr(p_i), ptr(s_i), _allowed_ptr(aa_allowed, mask_generate), N, L, stream()))
    return v_i, p_i, s_i


def add_noise(t, alpha_bars, fwd, noise, seed, offset, v_0, p_0, s_0, mask_generate, scale, mean,
              noise_structure=True, noise_sequence=True, grad_mode=False, want_eps=False, want_probs=False, seed_dev=None, aa_allowed=None):
    """fwd: ApproxAngularDistribution of the forward process (buffers stddevs, approx_flag, X + cdf()).  aa_allowed (optional): _allowed_ptr."""
    N, L = mask_generate.shape
    v_n, p_n, s_n = torch.empty_like(v_0), torch.empty_like(p_0), torch.empty_like(s_0)
    eps = torch.empty_like(p_0) if want_eps else None
    probs = torch.empty(N, L, 20, dtype=torch.float32, device=p_0.device) if want_probs else None
    nz = None
    if noise is not None:
        o = not noise_structure                  # sequence-only noising draws s_noisy alone (dpm_full.py:163-178)
        nz = AddNoiseNoise(ptr(noise.get('axis'), torch.float32, optional=o), ptr(noise.get('bin'), torch.int64, optional=o),
                           ptr(noise.get('ubin'), torch.float32, optional=o), ptr(noise.get('gauss'), torch.float32, optional=o),
                           ptr(noise.get('pos'), torch.float32, optional=o), ptr(noise.get('s_noisy'), torch.int64, optional=True))
    mean_arr = (C.c_float * 3)(*[float(m) for m in mean])
    cdf = fwd.cdf() if noise is None else None
    t, v_0, p_0, s_0, mask_generate = _contig(t, v_0, p_0, s_0, mask_generate)
    _check(lib().abopt_add_noise(ptr(t, torch.int64), ptr(alpha_bars, torch.float32), ptr(fwd.stddevs, torch.float32),
                                 ptr(fwd.approx_flag, torch.bool), ptr(fwd.X, torch.float32), ptr(cdf, optional=True), fwd.X.shape[1], fwd.X.shape[0],
                                 C.byref(nz) if nz is not None else None, seed, offset,
                                 ptr(v_0, torch.float32), ptr(p_0, torch.float32), ptr(s_0, torch.int64),
                                 ptr(mask_generate, torch.bool), float(scale), mean_arr, int(noise_structure), int(noise_sequence),
                                 int(grad_mode), ptr(v_n), ptr(p_n), ptr(s_n), ptr(eps, optional=True), ptr(probs, optional=True),
                                 ptr(seed_dev, torch.int64, optional=True), _allowed_ptr(aa_allowed, mask_generate), N, L, stream()))
    out = (v_n, p_n, s_n) + ((eps,) if want_eps else ()) + ((probs,) if want_probs else ())
    return out


def commonness_score(structs):
    structs = structs.contiguous().float()
    B, n, _ = structs.shape
    score = torch.empty(B, device=structs.device)
    _check(lib().abopt_commonness_score(ptr(structs), ptr(score), B, n, stream()))
    return score


def commonness_score_grouped(structs, group_size):
    """structs (G*S, n, 3), S = group_size -> (G*S,) commonness of every structure within its own group of S (abopt_commonness_score_grouped;
    row-for-row the bits of commonness_score called on each group)."""
    structs = structs.contiguous().float()
    B, n, _ = structs.shape
    S = int(group_size)
    if S < 2 or B % S:
        raise ValueError(f'commonness_score_grouped: {B} structures are not whole groups of {S} >= 2')
    score = torch.empty(B, device=structs.device)
    _check(lib().abopt_commonness_score_grouped(ptr(structs), ptr(score), B // S, S, n, stream()))
    return score


def check_cluster_cutoff(name, cutoff):
    """float(cutoff), or ValueError for a negative or non-finite one (the check abopt_cluster_poses_grouped makes, ahead of any device work)."""
    import math
    c = float(cutoff)
    if not math.isfinite(c) or c < 0.0:
        raise ValueError(f'{name} must be finite and >= 0 (got {cutoff!r})')
    return c


def cluster_poses_grouped(structs, group_size, cutoff, max_clusters=0, want_rmsd=False):
    """Greedy clustering of every group of S = group_size structures (include/abopt.h: abopt_cluster_poses_grouped).
    structs (G*S, n, 3); cutoff in Angstrom (RMSD without superposition); max_clusters 0 = no cap.
    -> dict of device tensors: label (G*S,) int32 (-1: left over at the cap), centre (G, S) int32 (indices within the group, -1 padded),
    size (G, S) int32 (0 padded), count (G,) int32 [, rmsd (G, S, S) fp32, symmetric bit for bit].  Two stream-ordered launches, no host synchronisation."""
    structs = structs.contiguous().float()
    B, n, _ = structs.shape
    S, M = int(group_size), int(max_clusters)
    if S < 1 or B % S or n < 1 or structs.shape[2] != 3:
        raise ValueError(f'cluster_poses_grouped: {tuple(structs.shape)} structures are not whole groups of {S} >= 1 structures (n, 3)')
    if M < 0:
        raise ValueError(f'cluster_poses_grouped: max_clusters must be >= 0 (0 = no cap), got {max_clusters!r}')
    cutoff = check_cluster_cutoff('cluster_poses_grouped: cutoff', cutoff)
    ptr(structs)                                                    # a CPU tensor is refused here, before anything is allocated
    G, dev = B // S, structs.device
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(label=torch.empty(B, **i32), centre=torch.empty(G, S, **i32), size=torch.empty(G, S, **i32), count=torch.empty(G, **i32))
    if want_rmsd:
        out['rmsd'] = torch.empty(G, S, S, dtype=torch.float32, device=dev)
    buf = Workspace.get(max(8, lib().abopt_cluster_ws_bytes(G, S)), dev)
    _check(lib().abopt_cluster_poses_grouped(ptr(structs), G, S, n, cutoff, M, ptr(buf), buf.numel(), ptr(out['label']), ptr(out['centre']), ptr(out['size']),
                                             ptr(out['count']), ptr(out.get('rmsd'), optional=True), stream()))
    return out


def cluster_shapes_grouped(structs, group_size, cutoff, max_clusters=0, want_rmsd=False):
    """`cluster_poses_grouped` with every pair of structures SUPERPOSED before the distance is taken: clusters by shape, whatever frame each structure lives in
    (include/abopt.h: abopt_cluster_shapes_grouped).  structs (G*S, n, 3) with 3 <= n <= 256 -- below three points no rotation is
    determined and the call refuses --; cutoff in Angstrom (RMSD after the best proper rotation and translation, all n points fitted and measured); max_clusters
    0 = no cap.  -> the dict of `cluster_poses_grouped`; rmsd (G, S, S) is symmetric bit for bit, 0 on the diagonal, and equals `superposed_rmsd` on rows
    (min, max) bit for bit.  Two stream-ordered launches, no host synchronisation."""
    structs = structs.contiguous().float()
    S, M = int(group_size), int(max_clusters)
    if structs.dim() != 3 or S < 1 or structs.shape[0] % S or structs.shape[2] != 3:
        raise ValueError(f'cluster_shapes_grouped: {tuple(structs.shape)} structures are not whole groups of {S} >= 1 structures (n, 3)')
    B, n, _ = structs.shape
    if not 3 <= n <= SIMILARITY_MAX_LEN:
        raise ValueError(f'cluster_shapes_grouped: structures have {n} points, expected 3 .. {SIMILARITY_MAX_LEN} (a best fit takes three)')
    if M < 0:
        raise ValueError(f'cluster_shapes_grouped: max_clusters must be >= 0 (0 = no cap), got {max_clusters!r}')
    cutoff = check_cluster_cutoff('cluster_shapes_grouped: cutoff', cutoff)
    ptr(structs)                                                    # a CPU tensor is refused here, before anything is allocated
    G, dev = B // S, structs.device
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(label=torch.empty(B, **i32), centre=torch.empty(G, S, **i32), size=torch.empty(G, S, **i32), count=torch.empty(G, **i32))
    if want_rmsd:
        out['rmsd'] = torch.empty(G, S, S, dtype=torch.float32, device=dev)
    buf = Workspace.get(max(8, lib().abopt_cluster_ws_bytes(G, S)), dev)
    _check(lib().abopt_cluster_shapes_grouped(ptr(structs), G, S, n, cutoff, M, ptr(buf), buf.numel(), ptr(out['label']), ptr(out['centre']), ptr(out['size']),
                                              ptr(out['count']), ptr(out.get('rmsd'), optional=True), stream()))
    return out


def check_max_mismatch(name, m):
    """int(m), or ValueError for a negative one (the check abopt_cluster_sequences_grouped makes, ahead of any device work)."""
    if isinstance(m, bool) or int(m) != m or int(m) < 0:
        raise ValueError(f'{name} must be an integer >= 0 (got {m!r})')
    return int(m)


def _seq_bytes(name, seqs, group_size):
    """(G*S, n) integer sequences on the device -> (uint8 bytes (G*S, n), G, S, n).  Values are brought into 0..255 by clamping, on the device (no host read):
    the kernels take one byte per residue type, and a value outside 0..255 saturates instead of wrapping onto a type."""
    S = int(group_size)
    if seqs.dim() != 2 or S < 1 or seqs.shape[0] % S or seqs.shape[1] < 1 or seqs.dtype.is_floating_point or seqs.dtype.is_complex:
        raise ValueError(f'{name}: {tuple(seqs.shape)} {seqs.dtype} sequences are not whole groups of {S} >= 1 integer sequences (n,)')
    ptr(seqs, strided=True)                                         # a CPU tensor is refused here, before anything is allocated
    b = seqs if seqs.dtype == torch.uint8 else (seqs.to(torch.uint8) if seqs.dtype == torch.bool else seqs.clamp(0, 255).to(torch.uint8))
    return b.contiguous(), seqs.shape[0] // S, S, seqs.shape[1]


def cluster_sequences_grouped(seqs, group_size, max_mismatch, max_clusters=0, want_dist=False):
    """Greedy clustering of every group of S = group_size sequences (include/abopt.h: abopt_cluster_sequences_grouped).
    seqs (G*S, n), any integer dtype, one residue type per entry (clamped into 0..255); a and b are neighbours iff they differ at no more than max_mismatch
    positions; max_clusters 0 = no cap.
    -> dict of device tensors: label (G*S,) int32 (-1: left over at the cap), centre (G, S) int32 (indices within the group, -1 padded),
    size (G, S) int32 (0 padded), count (G,) int32 [, dist (G, S, S) int32, symmetric].  Two stream-ordered launches, no host synchronisation."""
    M = int(max_clusters)
    if M < 0:
        raise ValueError(f'cluster_sequences_grouped: max_clusters must be >= 0 (0 = no cap), got {max_clusters!r}')
    m = check_max_mismatch('cluster_sequences_grouped: max_mismatch', max_mismatch)
    seqs, G, S, n = _seq_bytes('cluster_sequences_grouped', seqs, group_size)
    dev = seqs.device
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(label=torch.empty(G * S, **i32), centre=torch.empty(G, S, **i32), size=torch.empty(G, S, **i32), count=torch.empty(G, **i32))
    if want_dist:
        out['dist'] = torch.empty(G, S, S, **i32)
    buf = Workspace.get(max(8, lib().abopt_cluster_ws_bytes(G, S)), dev)
    _check(lib().abopt_cluster_sequences_grouped(ptr(seqs), G, S, n, min(m, 0x7fffffff), M, ptr(buf), buf.numel(), ptr(out['label']), ptr(out['centre']),
                                                 ptr(out['size']), ptr(out['count']), ptr(out.get('dist'), optional=True), stream()))
    return out


def sequence_profile_grouped(seqs, group_size):
    """Per-position composition of every group of S = group_size sequences (include/abopt.h: abopt_sequence_profile_grouped).
    seqs (G*S, n) as for cluster_sequences_grouped -> counts (G, n, 21) int32 on the device: bin t < 20 counts type t, bin 20 everything else; every position
    sums to S.  One stream-ordered launch."""
    seqs, G, S, n = _seq_bytes('sequence_profile_grouped', seqs, group_size)
    counts = torch.empty(G, n, 21, dtype=torch.int32, device=seqs.device)
    _check(lib().abopt_sequence_profile_grouped(ptr(seqs), G, S, n, ptr(counts), stream()))
    return counts


def check_distance_cutoff(name, v):
    """float(v), or ValueError for a negative or non-finite one (the check abopt_interface_geometry_grouped makes on its cutoffs, ahead of any device work)."""
    import math
    c = float(v)
    if not math.isfinite(c) or c < 0.0:
        raise ValueError(f'{name} must be finite and >= 0 (got {v!r})')
    return c


def _candidate_args(name, pos, mask, group):
    """The shape contract of the scorers that compare the two sides of `group`, checked without a device: group (G, L), pos (G*S, L, A, 3) in whole groups of S,
    mask (G*S, L, A) or (G, L, A) shared by the candidates of a group, 1 <= A <= 15.  -> (G, S, L, A, shared: the mask is per group), or ValueError."""
    if group.dim() != 2 or pos.dim() != 4 or mask.dim() != 3:
        raise ValueError(f'{name}: expected pos (G*S, L, A, 3), mask (G*S or G, L, A) and group (G, L), got {tuple(pos.shape)}, '
                         f'{tuple(mask.shape)} and {tuple(group.shape)}')
    G, L = group.shape
    N, A = pos.shape[0], pos.shape[2]
    if L < 1 or tuple(pos.shape[1:]) != (L, A, 3) or (N % G if G else N):
        raise ValueError(f'{name}: {tuple(pos.shape)} candidates are not whole groups of the {G} rows of group {tuple(group.shape)}')
    if not 1 <= A <= 15:
        raise ValueError(f'{name}: A={A} atoms per residue, expected 1 .. 15')
    S = N // G if G else 0
    shared = mask.shape[0] != N or S == 1
    if tuple(mask.shape) != ((G if shared else N), L, A):
        raise ValueError(f'{name}: mask {tuple(mask.shape)} is neither per candidate nor per group')
    return G, S, L, A, shared


def _as_flags(t):
    """a per-residue or per-atom flag tensor as contiguous bool or uint8 (None stays None)"""
    return None if t is None else (t if t.dtype in (torch.bool, torch.uint8) else t != 0).contiguous()


def _candidate_tensors(pos, mask, group, link=None):
    """What the entry points of those scorers read: pos as contiguous fp32, mask and link (None stays None) as contiguous bool or uint8, group as contiguous int32
    (None -- a caller whose rows are flags, not sides -- stays None).  A CPU tensor is refused first, before anything is allocated.  -> (pos, mask, group, link)"""
    ptr(pos, strided=True)
    return pos.float().contiguous(), _as_flags(mask), None if group is None else group.to(torch.int32).contiguous(), _as_flags(link)


def interface_geometry_grouped(pos, mask, group, clash_cutoff=3.0, contact_cutoff=5.0, link=None, bond_max=None, want_freq=False):
    """Clashes, contacts, interface residues and chain breaks of G*S candidates in G groups (include/abopt.h: abopt_interface_geometry_grouped; DESIGN.md
    section 6.3).  pos (G*S,L,A,3); mask (G*S,L,A), or (G,L,A) shared by the S candidates of a group; group (G,L) int: 1 and 2 name the two sides, anything else
    takes no part; link (optional, (G,L) bool): residue r is peptide-bonded to r + 1 -- bonded neighbours are not compared, and with bond_max (Angstrom; None:
    breaks are not counted) a link whose C-N distance exceeds it is a break.  Cutoffs in Angstrom: clash d < clash_cutoff per atom pair, contact
    min d <= contact_cutoff per residue pair.
    -> dict of device tensors: clash, contacts, iface1, iface2, breaks (G*S,) int32 [, freq (G,L) int32 with want_freq: in how many of the group's candidates
    each residue is in a contact].  Stream-ordered, no host synchronisation."""
    name = 'interface_geometry_grouped'
    G, S, L, A, shared = _candidate_args(name, pos, mask, group)
    if link is not None and (tuple(link.shape) != (G, L) or A < 3):
        raise ValueError(f'{name}: link {tuple(link.shape)} must be (G, L) = {(G, L)} and needs the backbone atoms (A >= 3, got {A})')
    clash = check_distance_cutoff(f'{name}: clash_cutoff', clash_cutoff)
    contact = check_distance_cutoff(f'{name}: contact_cutoff', contact_cutoff)
    bond = -1.0 if bond_max is None else check_distance_cutoff(f'{name}: bond_max', bond_max)
    pos, mask, group, link = _candidate_tensors(pos, mask, group, link)
    N, dev = G * S, pos.device
    out = torch.empty(N, 5, dtype=torch.int32, device=dev)
    freq = (torch.empty if N else torch.zeros)(G, L, dtype=torch.int32, device=dev) if want_freq else None      # an empty call launches nothing
    buf = Workspace.get(max(8, lib().abopt_interface_geometry_ws_bytes(G, S, L)), dev)
    _check(lib().abopt_interface_geometry_grouped(ptr(pos, torch.float32), ptr(mask), int(shared), ptr(group, torch.int32), ptr(link, optional=True), G, S, L, A,
                                                  clash, contact, bond, ptr(out), ptr(freq, optional=True), ptr(buf), buf.numel(), stream()))
    res = dict(zip(('clash', 'contacts', 'iface1', 'iface2', 'breaks'), out.unbind(1)))
    if want_freq:
        res['freq'] = freq
    return res


RELAX_MAX_ITERS = 1024      # iterations of one call at most
RELAX_MAX_MOVED = 256       # moved residues of one candidate at most (abopt_relax_max_moved(): what fits the LDS of a workgroup with 15 atom slots)


def check_relax(w_bond=1.0, w_ca=1.0, w_clash=1.0, w_tether=0.05, clash_cutoff=3.0, step=0.2, max_shift=0.5, max_angle=0.2, iters=50, max_moved=None):
    """The knobs of the relax (include/abopt.h: abopt_relax_grouped) as a dict under their own names -- floats, iters and max_moved (None
    stays None) as ints --, or ValueError naming the argument: every scalar finite and >= 0, max_shift and max_angle > 0, iters 0 .. 1024, max_moved 1 ..
    RELAX_MAX_MOVED.  No device is needed."""
    import math
    out = {}
    for name, v in (('w_bond', w_bond), ('w_ca', w_ca), ('w_clash', w_clash), ('w_tether', w_tether), ('clash_cutoff', clash_cutoff), ('step', step),
                    ('max_shift', max_shift), ('max_angle', max_angle)):
        f = float(v)
        if not math.isfinite(f) or f < 0.0:
            raise ValueError(f'{name} must be finite and >= 0 (got {v!r})')
        out[name] = f
    for name in ('max_shift', 'max_angle'):
        if out[name] == 0.0:
            raise ValueError(f'{name} must be > 0')
    if isinstance(iters, bool) or int(iters) != iters or not 0 <= int(iters) <= RELAX_MAX_ITERS:
        raise ValueError(f'iters must be an integer in 0 .. {RELAX_MAX_ITERS} (got {iters!r})')
    out['iters'] = int(iters)
    if max_moved is not None and (isinstance(max_moved, bool) or int(max_moved) != max_moved or not 1 <= int(max_moved) <= RELAX_MAX_MOVED):
        raise ValueError(f'max_moved must be an integer in 1 .. {RELAX_MAX_MOVED} (got {max_moved!r})')
    out['max_moved'] = None if max_moved is None else int(max_moved)
    return out


def relax_grouped(pos, mask, move, link=None, w_bond=1.0, w_ca=1.0, w_clash=1.0, w_tether=0.05, clash_cutoff=3.0, step=0.2, max_shift=0.5, max_angle=0.2,
                  iters=50, out=None, max_moved=None):
    """Relax G*S candidates in G groups: `iters` Jacobi steps of a rigid-residue descent on atom-level clashes, peptide-bond and CA-CA violations, tethered to
    the input (include/abopt.h: abopt_relax_grouped).  pos (G*S,L,A,3) with atom slots 0, 1, 2 = N, CA, C (3 <= A <= 15); mask (G*S,L,A), or
    (G,L,A) shared by the S candidates of a group; move (G,L) bool: the residues that may move; link (optional, (G,L) bool): residue r is peptide-bonded to
    r + 1 -- without it there is no bond term, no CA term and no neighbour exclusion.  Weights are per squared Angstrom, clash_cutoff / max_shift in Angstrom,
    max_angle in rad.  The defaults are conventional values (3 A between heavy atoms, half an Angstrom and a fifth of a radian per step), NOT tuned ones: no
    trained checkpoint exists to tune them on.  out (optional): the tensor the result is written to, contiguous fp32 of pos's shape -- pos itself relaxes in place.
    max_moved (optional): the caller's bound on the moved residues of any one candidate, at most RELAX_MAX_MOVED; it sizes the workgroup's LDS (default
    min(L, RELAX_MAX_MOVED)).  A candidate with more moved residues than the bound comes back unchanged with NaN energies -- the count lives on the device and no
    host read is made for it.
    -> dict of device tensors: pos (G*S,L,A,3) fp32 and energy (G*S,2,4) fp32: bond, ca, clash, tether before and after.  Stream-ordered, no host
    synchronisation, capturable in a torch.cuda.graph."""
    name = 'relax_grouped'
    ptr(pos, strided=True)                                          # a CPU tensor is refused here, before anything else
    kn = check_relax(w_bond, w_ca, w_clash, w_tether, clash_cutoff, step, max_shift, max_angle, iters, max_moved)
    G, S, L, A, shared = _candidate_args(name, pos, mask, move)
    if A < 3:
        raise ValueError(f'{name}: A={A} atoms per residue, the slots 0, 1, 2 are N, CA, C (expected 3 .. 15)')
    if link is not None and tuple(link.shape) != (G, L):
        raise ValueError(f'{name}: link {tuple(link.shape)} must be (G, L) = {(G, L)}')
    src, mask, _, link = _candidate_tensors(pos, mask, None, link)
    move = _as_flags(move)
    if out is None:
        out = torch.empty_like(src)
    elif out.shape != src.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != src.device:
        raise ValueError(f'{name}: out must be a contiguous fp32 tensor of shape {tuple(src.shape)} on {src.device}')
    N, dev = G * S, src.device
    energy = (torch.empty if N else torch.zeros)(N, 2, 4, dtype=torch.float32, device=dev)       # an empty call launches nothing
    _check(lib().abopt_relax_grouped(ptr(src, torch.float32), ptr(out, torch.float32), ptr(mask), int(shared), ptr(move), ptr(link, optional=True), G, S, L, A,
                                     kn['max_moved'] or min(L, RELAX_MAX_MOVED), kn['w_bond'], kn['w_ca'], kn['w_clash'], kn['w_tether'], kn['clash_cutoff'],
                                     kn['step'], kn['max_shift'], kn['max_angle'], kn['iters'], ptr(energy, torch.float32), stream()))
    return dict(pos=out, energy=energy)


def check_probe_radius(name, v):
    """float(v), or ValueError for a negative or non-finite one (the check abopt_sasa_grouped makes on its probe radius, ahead of any device work)."""
    import math
    c = float(v)
    if not math.isfinite(c) or c < 0.0:
        raise ValueError(f'{name} must be finite and >= 0 (got {v!r})')
    return c


_SPHERE_POINTS = {}


def sphere_points(n, device='cpu'):
    """n unit vectors spread over the sphere by the golden-section spiral: z_k = 1 - (2 k + 1) / n, rho = sqrt(1 - z^2), phi = k pi (3 - sqrt 5),
    (rho cos phi, rho sin phi, z) -- computed in float64 on the host and rounded to fp32 once.  -> (n, 3) fp32 on `device`, cached per (n, device): treat it as
    read-only."""
    import math
    n = int(n)
    if not 1 <= n <= 1024:
        raise ValueError(f'sphere_points: n={n} test points, expected 1 .. 1024')
    key = (n, str(torch.device(device)))
    if key not in _SPHERE_POINTS:
        k = torch.arange(n, dtype=torch.float64)
        z = 1.0 - (2.0 * k + 1.0) / n
        rho = torch.sqrt(1.0 - z * z)
        phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
        _SPHERE_POINTS[key] = torch.stack([rho * torch.cos(phi), rho * torch.sin(phi), z], 1).float().to(device)
    return _SPHERE_POINTS[key]


def sasa_grouped(pos, mask, group, radius, probe=1.4, points=128):
    """Shrake-Rupley surface of G*S candidates in G groups, free and in the complex (include/abopt.h: abopt_sasa_grouped).
    pos (G*S,L,A,3); mask (G*S,L,A), or (G,L,A) shared by the S candidates of a group; group (G,L) int: 1 and 2 name the two sides, anything else takes no part
    (neither scored nor an occluder); radius (G,L,A), or (L,A) or (A,) broadcast to it: the van der Waals radius per atom slot in Angstrom, 0 (or NaN, or > 16) =
    the slot takes no part; probe in Angstrom; points: test points per atom (`sphere_points`), 1 .. 1024.
    -> dict of device tensors: pts (G*S,4) int32 (free-exposed points of side 1, of side 2, complex-exposed points of side 1, of side 2) and area (G*S,L,2) fp32
    (free and complex exposed area per residue; their difference is the buried area).  Stream-ordered, no host synchronisation, capturable in a torch.cuda.graph."""
    import math
    G, S, L, A, shared = _candidate_args('sasa_grouped', pos, mask, group)
    if tuple(radius.shape) not in ((G, L, A), (L, A), (A,)):
        raise ValueError(f'sasa_grouped: radius {tuple(radius.shape)} must be (G, L, A) = {(G, L, A)}, (L, A) or (A,)')
    n = int(points)
    if not 1 <= n <= 1024:
        raise ValueError(f'sasa_grouped: points={points!r} test points per atom, expected 1 .. 1024')
    probe = check_probe_radius('sasa_grouped: probe', probe)
    pos, mask, group, _ = _candidate_tensors(pos, mask, group)
    N, dev = G * S, pos.device
    radius = radius.to(device=dev, dtype=torch.float32).expand(G, L, A).contiguous()
    dirs = sphere_points(n, dev)
    k = float(torch.tensor(4.0 * math.pi / n, dtype=torch.float64).float())       # float32(4 pi / n) from float64
    pts = (torch.empty if N else torch.zeros)(N, 4, dtype=torch.int32, device=dev)         # an empty call launches nothing
    area = (torch.empty if N else torch.zeros)(N, L, 2, dtype=torch.float32, device=dev)
    buf = Workspace.get(max(16, lib().abopt_sasa_ws_bytes(G, S, L, A)), dev)
    _check(lib().abopt_sasa_grouped(ptr(pos, torch.float32), ptr(mask), int(shared), ptr(group, torch.int32), ptr(radius, torch.float32), ptr(dirs, torch.float32),
                                    n, G, S, L, A, probe, k, ptr(pts), ptr(area), ptr(buf), buf.numel(), stream()))
    return dict(pts=pts, area=area)


LIABILITY_RUN_MAX = 16      # the longest hydrophobic-run window


def check_run_min(name, v):
    """int(v): 0 (the hydrophobic-run class is off) or 2 .. 16, or ValueError (the check abopt_sequence_liabilities_grouped makes, ahead of any device work)."""
    if isinstance(v, bool) or int(v) != v or not (int(v) == 0 or 2 <= int(v) <= LIABILITY_RUN_MAX):
        raise ValueError(f'{name} must be 0 (off) or an integer in 2 .. {LIABILITY_RUN_MAX} (got {v!r})')
    return int(v)


def sequence_liabilities_grouped(seqs, group_size, rows=None, link=None, run_min=5, want_freq=False):
    """Sequence liabilities of G*S designs in G groups (include/abopt.h: abopt_sequence_liabilities_grouped).  seqs (G*S, n) as for
    cluster_sequences_grouped (type k = model.AA_LETTERS[k]; a byte >= 20 is no type); rows (optional, (G, n) bool): the scored positions, None = all; link
    (optional, (G, n) bool): residue k is peptide-bonded to k + 1 (`sampler.backbone_links`), None = every consecutive pair; run_min: the length of a
    hydrophobic run, 0 = off, else 2 .. 16.  A motif window exists iff it lies inside the sequence, every step of it is linked and every byte is a type; it
    counts iff one of its positions is a scored row.
    -> dict of device tensors: flags (G*S, n) uint8, bit b at a window's anchor = class model.LIABILITY_NAMES[b]; counts (G*S, 12) int32: the windows counted
    per class (0-6), the flagged positions (7), K + R, D + E, H among the scored rows (8-10), the scored rows that hold a type (11); hyd10 (G*S,) int32: ten
    times the Kyte-Doolittle hydropathy summed over the scored rows [, freq (G, n) int32 with want_freq: how many of the group's designs carry a flag at each
    position].  One stream-ordered launch, no host synchronisation, capturable."""
    name = 'sequence_liabilities_grouped'
    run = check_run_min(f'{name}: run_min', run_min)
    if seqs.dim() == 2 and int(group_size) >= 1 and seqs.shape[0] % int(group_size) == 0:
        want = (seqs.shape[0] // int(group_size), seqs.shape[1])
        for what, t in (('rows', rows), ('link', link)):
            if t is not None and tuple(t.shape) != want:
                raise ValueError(f'{name}: {what} {tuple(t.shape)} must be (G, n) = {want}')
    seqs, G, S, n = _seq_bytes(name, seqs, group_size)
    rows, link = _as_flags(rows), _as_flags(link)
    N, dev = G * S, seqs.device
    new = torch.empty if N else torch.zeros                          # an empty call launches nothing
    flags = new(N, n, dtype=torch.uint8, device=dev)
    counts = new(N, 13, dtype=torch.int32, device=dev)
    freq = new(G, n, dtype=torch.int32, device=dev) if want_freq else None
    _check(lib().abopt_sequence_liabilities_grouped(ptr(seqs), ptr(rows, optional=True), ptr(link, optional=True), run, G, S, n, ptr(flags), ptr(counts),
                                                    ptr(freq, optional=True), stream()))
    res = dict(flags=flags, counts=counts[:, :12], hyd10=counts[:, 12])
    if want_freq:
        res['freq'] = freq
    return res


_PATCH_WEIGHT = {}


def default_patch_weight(device='cpu'):
    """The default hydrophobicity table of `surface_patches_grouped`: the Kyte-Doolittle hydropathy of the twenty types (model.KD_HYDROPATHY, each rounded to fp32
    once) and 0 for entry 20, which serves every byte >= 20.  -> (21,) fp32 on `device`, cached per device: treat it as read-only."""
    key = str(torch.device(device))
    if key not in _PATCH_WEIGHT:
        from .model import KD_HYDROPATHY
        _PATCH_WEIGHT[key] = torch.tensor(list(KD_HYDROPATHY) + [0.0], dtype=torch.float64).float().to(device)
    return _PATCH_WEIGHT[key]


def surface_patches_grouped(pos, mask, group, area, seqs, weight=None, radius=10.0):
    """Exposed hydrophobic patches of G*S candidates in G groups (include/abopt.h: abopt_surface_patches_grouped): per residue of side 1,
    the sum of weight[type] x exposed area over the side-1 residues whose centre (CB, else CA) lies within `radius` of its own.  pos (G*S,L,A,3), 2 <= A <= 15;
    mask (G*S,L,A), or (G,L,A) shared by the S candidates of a group; group (G,L) int: only side 1 is scored and contributes; area (G*S,L): the exposed area per
    residue, e.g. a column of sasa_grouped's area; seqs (G*S,L), or (G,L) shared by the group, any integer dtype (clamped into 0..255; a byte >= 20 reads
    weight[20]); weight (optional, (21,)): default `default_patch_weight` (Kyte-Doolittle, 0 for entry 20) -- a NaN entry takes that type out; radius in Angstrom.
    -> dict of device tensors: patch (G*S,L) fp32 and nbr (G*S,L) int32 (the residue itself included; both 0 for a residue that takes no part).  One
    stream-ordered launch, no host synchronisation, capturable."""
    name = 'surface_patches_grouped'
    G, S, L, A, shared = _candidate_args(name, pos, mask, group)
    if A < 2:
        raise ValueError(f'{name}: A={A} atoms per residue, the slot 1 is CA (expected 2 .. 15)')
    N = G * S
    if tuple(area.shape) != (N, L) or not area.dtype.is_floating_point:
        raise ValueError(f'{name}: area {tuple(area.shape)} {area.dtype} must be floating point of shape (G*S, L) = {(N, L)}')
    if seqs.dim() != 2 or seqs.shape[1] != L or seqs.shape[0] not in (N, G) or seqs.dtype.is_floating_point or seqs.dtype.is_complex:
        raise ValueError(f'{name}: seqs {tuple(seqs.shape)} {seqs.dtype} must be integer of shape (G*S, L) = {(N, L)} or (G, L) = {(G, L)}')
    if weight is not None and (tuple(weight.shape) != (21,) or not weight.dtype.is_floating_point):
        raise ValueError(f'{name}: weight {tuple(weight.shape)} {weight.dtype} must be floating point of shape (21,): the twenty types and "no type"')
    radius = check_distance_cutoff(f'{name}: radius', radius)
    pos, mask, group, _ = _candidate_tensors(pos, mask, group)
    dev = pos.device
    seq_shared = seqs.shape[0] != N or S == 1
    seqs = (seqs if seqs.dtype == torch.uint8 else seqs.to(torch.uint8) if seqs.dtype == torch.bool else seqs.clamp(0, 255).to(torch.uint8)).contiguous()
    area = area.float().contiguous()
    weight = default_patch_weight(dev) if weight is None else weight.to(device=dev, dtype=torch.float32).contiguous()
    new = torch.empty if N else torch.zeros                          # an empty call launches nothing
    patch = new(N, L, dtype=torch.float32, device=dev)
    nbr = new(N, L, dtype=torch.int32, device=dev)
    _check(lib().abopt_surface_patches_grouped(ptr(pos, torch.float32), ptr(mask), int(shared), ptr(group, torch.int32), ptr(area, torch.float32), ptr(seqs, torch.uint8),
                                               int(seq_shared), ptr(weight, torch.float32), radius, G, S, L, A, ptr(patch), ptr(nbr), stream()))
    return dict(patch=patch, nbr=nbr)


_RESIDUE_CHARGE = {}


def default_residue_charge(device='cpu'):
    """The default charge table of `interface_energy_grouped`: model.RESIDUE_CHARGE (K, R = +1; D, E = -1; everything else and entry 20 are 0).
    -> (21,) fp32 on `device`, cached per device: treat it as read-only."""
    key = str(torch.device(device))
    if key not in _RESIDUE_CHARGE:
        from .model import RESIDUE_CHARGE
        _RESIDUE_CHARGE[key] = torch.tensor(RESIDUE_CHARGE, dtype=torch.float32).to(device)
    return _RESIDUE_CHARGE[key]


def check_interface_energy(hb_cutoff=-0.5, elec_cutoff=15.0, salt_cutoff=7.0, pair_cutoff=8.0, eps=4.0, d_min=3.0):
    """The knobs of the interface energy (include/abopt.h: abopt_interface_energy_grouped) as a dict of floats under their own names, or
    ValueError naming the argument: hb_cutoff finite and <= 0 (kcal/mol), the three cutoffs finite and >= 0 (Angstrom), eps and d_min finite and > 0.  The
    defaults are conventional values (DSSP's -0.5 kcal/mol; 15, 7 and 8 A; eps = 4 r; a floor of 3 A), NOT tuned ones.  No device is needed."""
    import math
    out = {}
    f = float(hb_cutoff)
    if not math.isfinite(f) or f > 0.0:
        raise ValueError(f'hb_cutoff must be finite and <= 0 (got {hb_cutoff!r})')
    out['hb_cutoff'] = f
    for name, v in (('elec_cutoff', elec_cutoff), ('salt_cutoff', salt_cutoff), ('pair_cutoff', pair_cutoff), ('eps', eps), ('d_min', d_min)):
        f = float(v)
        if not math.isfinite(f) or f < 0.0:
            raise ValueError(f'{name} must be finite and >= 0 (got {v!r})')
        if name in ('eps', 'd_min') and f == 0.0:
            raise ValueError(f'{name} must be > 0')
        out[name] = f
    return out


def interface_energy_grouped(pos, mask, group, seqs, charge=None, pair_table=None, link=None, **knobs):
    """Interface energetics of G*S candidates in G groups (include/abopt.h: abopt_interface_energy_grouped): per residue of either side,
    over its partners on the other side, backbone hydrogen bonds (the DSSP rule), a Coulomb term between charged centres (CB, else CA) with the dielectric eps r,
    and a caller's pair table within pair_cutoff.  pos (G*S,L,A,3), 4 <= A <= 15, slots 0 .. 4 = N, CA, C, O, CB; mask (G*S,L,A), or (G,L,A) shared by the S
    candidates of a group; group (G,L) int: 1 and 2 name the two sides; seqs (G*S,L), or (G,L) shared by the group, any integer dtype (clamped into 0..255; a
    byte >= 20 reads entry 20 of both tables); charge (optional, (21,)): default `default_residue_charge` -- a NaN entry takes that type out; pair_table
    (optional, (21,21)): None = the pair term is off (model.hydrophobic_contact_table() is a placeholder, no statistical potential is shipped); link (optional,
    (G,L) bool, `sampler.backbone_links`): residue r is peptide-bonded to r + 1, None = every consecutive pair.  knobs: those of `check_interface_energy`,
    conventional values, not tuned ones.
    -> dict of device tensors: energy (G*S,L,3) fp32 (hb, elec, pair; kcal/mol-like) and count (G*S,L,5) int32 (bonds as donor, as acceptor, salt bridges,
    like-charge pairs, partners within pair_cutoff); zeros for a residue on no side.  A pair's energy is given in full to both residues: per-candidate totals sum
    one side (`sampler.energy_summary`).  One stream-ordered launch, no host synchronisation, capturable."""
    name = 'interface_energy_grouped'
    kn = check_interface_energy(**knobs)
    G, S, L, A, shared = _candidate_args(name, pos, mask, group)
    if A < 4:
        raise ValueError(f'{name}: A={A} atoms per residue, the slots 0 .. 3 are N, CA, C, O (expected 4 .. 15)')
    N = G * S
    if seqs.dim() != 2 or seqs.shape[1] != L or seqs.shape[0] not in (N, G) or seqs.dtype.is_floating_point or seqs.dtype.is_complex:
        raise ValueError(f'{name}: seqs {tuple(seqs.shape)} {seqs.dtype} must be integer of shape (G*S, L) = {(N, L)} or (G, L) = {(G, L)}')
    if charge is not None and (tuple(charge.shape) != (21,) or not charge.dtype.is_floating_point):
        raise ValueError(f'{name}: charge {tuple(charge.shape)} {charge.dtype} must be floating point of shape (21,): the twenty types and "no type"')
    if pair_table is not None and (tuple(pair_table.shape) != (21, 21) or not pair_table.dtype.is_floating_point):
        raise ValueError(f'{name}: pair_table {tuple(pair_table.shape)} {pair_table.dtype} must be floating point of shape (21, 21)')
    if link is not None and tuple(link.shape) != (G, L):
        raise ValueError(f'{name}: link {tuple(link.shape)} must be (G, L) = {(G, L)}')
    pos, mask, group, link = _candidate_tensors(pos, mask, group, link)
    dev = pos.device
    seq_shared = seqs.shape[0] != N or S == 1
    seqs = (seqs if seqs.dtype == torch.uint8 else seqs.to(torch.uint8) if seqs.dtype == torch.bool else seqs.clamp(0, 255).to(torch.uint8)).contiguous()
    charge = default_residue_charge(dev) if charge is None else charge.to(device=dev, dtype=torch.float32).contiguous()
    if pair_table is not None:
        pair_table = pair_table.to(device=dev, dtype=torch.float32).contiguous()
    new = torch.empty if N else torch.zeros                          # an empty call launches nothing
    energy = new(N, L, 3, dtype=torch.float32, device=dev)
    count = new(N, L, 5, dtype=torch.int32, device=dev)
    _check(lib().abopt_interface_energy_grouped(ptr(pos, torch.float32), ptr(mask), int(shared), ptr(group, torch.int32), ptr(seqs, torch.uint8), int(seq_shared),
                                                ptr(link, optional=True), ptr(charge, torch.float32), ptr(pair_table, torch.float32, optional=True), G, S, L, A,
                                                kn['hb_cutoff'], kn['elec_cutoff'], kn['salt_cutoff'], kn['pair_cutoff'], kn['eps'], kn['d_min'], ptr(energy),
                                                ptr(count), stream()))
    return dict(energy=energy, count=count)


BACKBONE_MAX_ROWS = 512     # residues of one candidate at most (abopt_backbone_max_rows(): the hydrogen-bond relation lives in a workgroup's LDS)
BACKBONE_MAX_REGIONS = 8    # rows of a Ramachandran table
BACKBONE_COUNTS = ('part', 'phipsi') + tuple(f'region{k}' for k in range(8)) + ('outliers', 'outliers_gly', 'omega', 'cis', 'cis_nonpro', 'twisted', 'H', 'E',
                                                                                   'G', 'I', 'T', 'C', 'hb_donor', 'hb_acceptor')


def rama_regions(table=None):
    """A Ramachandran table in degrees -> the (K, 8) fp32 tensor (on the CPU) that `backbone_conformation_grouped` takes: per row cos, sin of phi_lo, phi_hi,
    psi_lo, psi_hi, computed in float64 and rounded once.  table: K <= 8 rows (phi_lo, phi_hi, psi_lo, psi_hi), each arc running counter-clockwise from lo to hi
    (angles are taken modulo 360); None = model.RAMA_REGIONS, this library's coarse three boxes (see there: not a published contour).  ValueError for an arc of
    0 degrees or of >= 180 degrees (the two half-plane tests of the definition describe an arc only below 180), for a non-finite bound and for K > 8.  No
    device is needed."""
    import math
    if table is None:
        from .model import RAMA_REGIONS as table
    rows = [tuple(float(v) for v in row) for row in table]
    if len(rows) > BACKBONE_MAX_REGIONS or any(len(row) != 4 for row in rows):
        raise ValueError(f'rama_regions: expected at most {BACKBONE_MAX_REGIONS} rows of (phi_lo, phi_hi, psi_lo, psi_hi), got {len(rows)} rows')
    out = torch.zeros(len(rows), 8, dtype=torch.float64)
    for k, row in enumerate(rows):
        if not all(math.isfinite(v) for v in row):
            raise ValueError(f'rama_regions: row {k} holds a non-finite bound: {row}')
        for name, lo, hi in (('phi', row[0], row[1]), ('psi', row[2], row[3])):
            width = (hi - lo) % 360.0
            if not 0.0 < width < 180.0:
                raise ValueError(f'rama_regions: row {k}: the {name} arc {lo} .. {hi} is {width} degrees wide, expected 0 < width < 180')
        for c, v in enumerate(row):
            out[k, 2 * c], out[k, 2 * c + 1] = math.cos(math.radians(v)), math.sin(math.radians(v))
    return out.float()


def check_backbone_conformation(L=1, A=4, regions=None, hb_cutoff=-0.5):
    """The values `backbone_conformation_grouped` checks besides its shapes, without a device: L <= BACKBONE_MAX_ROWS, 4 <= A <= 15, regions None or a (K, 8)
    floating-point tensor with K <= 8, hb_cutoff finite and <= 0 (kcal/mol; DSSP's -0.5 is the conventional value, not a tuned one).
    -> dict(K, hb_cutoff), or ValueError naming the argument."""
    import math
    if not 1 <= int(L) <= BACKBONE_MAX_ROWS:
        raise ValueError(f'L={L} residues, expected 1 .. {BACKBONE_MAX_ROWS} (the hydrogen-bond relation of a candidate lives in the LDS of one workgroup)')
    if not 4 <= int(A) <= 15:
        raise ValueError(f'A={A} atoms per residue, the slots 0 .. 3 are N, CA, C, O (expected 4 .. 15)')
    K = 0
    if regions is not None:
        if regions.dim() != 2 or regions.shape[1] != 8 or regions.shape[0] > BACKBONE_MAX_REGIONS or not regions.dtype.is_floating_point:
            raise ValueError(f'regions {tuple(regions.shape)} {regions.dtype} must be floating point of shape (K, 8) with K <= {BACKBONE_MAX_REGIONS} '
                             f'(hip.rama_regions makes one)')
        K = regions.shape[0]
    f = float(hb_cutoff)
    if not math.isfinite(f) or f > 0.0:
        raise ValueError(f'hb_cutoff must be finite and <= 0 (got {hb_cutoff!r})')
    return dict(K=K, hb_cutoff=f)


def backbone_conformation_grouped(pos, mask, rows, seqs=None, link=None, regions=None, hb_cutoff=-0.5):
    """Backbone conformation of G*S candidates in G groups (include/abopt.h: abopt_backbone_conformation_grouped): per scored residue
    phi, psi, omega as (cos, sin), the peptide bond's length and two angle cosines, a Ramachandran class, and DSSP-LIKE states from Kabsch & Sander's hydrogen-bond
    patterns within the candidate (NOT DSSP: no ladders or sheets, no B / E distinction, no bends, no helix trimming); per candidate 24 counts.
    pos (G*S,L,A,3), 4 <= A <= 15, slots 0 .. 3 = N, CA, C, O, L <= 512; mask (G*S,L,A), or (G,L,A) shared by the S candidates of a group; rows (G,L) flags: the
    scored residues (every residue is a neighbour and a hydrogen-bond partner all the same); seqs (optional; (G*S,L), or (G,L) shared by the group, any integer
    dtype, clamped into 0..255): only Pro (12) and Gly (5) matter, None = no residue is either; link (optional, (G,L) bool, `sampler.backbone_links`): residue
    r is peptide-bonded to r + 1, None = every consecutive pair; regions (optional, (K,8), `rama_regions`): None = rama_regions() of model.RAMA_REGIONS, a
    (0,8) tensor = no region, every residue with phi and psi an outlier; hb_cutoff in kcal/mol.
    -> dict of device tensors: torsion (G*S,L,6) fp32 (cos, sin of phi, psi, omega; 0 where undefined), have (G*S,L) uint8 (bits 0 .. 2 phi, psi, omega; 3 .. 5
    the entries of bond), bond (G*S,L,3) fp32 (|C - N'|, cos CA-C-N', cos C-N'-CA' of the step r -> r + 1), rama (G*S,L) uint8 (region, K = outlier, 255 = none),
    ss (G*S,L) uint8 (bits: helix_4, helix_3, helix_5, parallel bridge, antiparallel bridge, inside a turn), state (G*S,L) uint8 (index into model.SS_LETTERS,
    255 = not scored), partner (G*S,L,2) int32 (lowest parallel / antiparallel bridge partner or -1), count (G*S,24) int32 (columns: BACKBONE_COUNTS).  One
    stream-ordered launch, no host synchronisation, capturable."""
    name = 'backbone_conformation_grouped'
    G, S, L, A, shared = _candidate_args(name, pos, mask, rows)
    try:
        kn = check_backbone_conformation(L, A, regions, hb_cutoff)
    except ValueError as e:
        raise ValueError(f'{name}: {e}') from None
    N = G * S
    if seqs is not None and (seqs.dim() != 2 or seqs.shape[1] != L or seqs.shape[0] not in (N, G) or seqs.dtype.is_floating_point or seqs.dtype.is_complex):
        raise ValueError(f'{name}: seqs {tuple(seqs.shape)} {seqs.dtype} must be integer of shape (G*S, L) = {(N, L)} or (G, L) = {(G, L)}')
    if link is not None and tuple(link.shape) != (G, L):
        raise ValueError(f'{name}: link {tuple(link.shape)} must be (G, L) = {(G, L)}')
    pos, mask, _, link = _candidate_tensors(pos, mask, None, link)
    dev = pos.device
    rows = _as_flags(rows)
    seq_shared = seqs is not None and (seqs.shape[0] != N or S == 1)
    if seqs is not None:
        seqs = (seqs if seqs.dtype == torch.uint8 else seqs.to(torch.uint8) if seqs.dtype == torch.bool else seqs.clamp(0, 255).to(torch.uint8)).contiguous()
    regions = (_rama_default(dev) if regions is None else regions.to(device=dev, dtype=torch.float32).contiguous())
    K = regions.shape[0]
    new = torch.empty if N else torch.zeros                          # an empty call launches nothing
    u8, i32, f32 = (dict(dtype=t, device=dev) for t in (torch.uint8, torch.int32, torch.float32))
    out = dict(torsion=new(N, L, 6, **f32), have=new(N, L, **u8), bond=new(N, L, 3, **f32), rama=new(N, L, **u8), ss=new(N, L, **u8), state=new(N, L, **u8),
               partner=new(N, L, 2, **i32), count=new(N, len(BACKBONE_COUNTS), **i32))
    _check(lib().abopt_backbone_conformation_grouped(ptr(pos, torch.float32), ptr(mask), int(shared), ptr(rows), ptr(seqs, torch.uint8, optional=True),
                                                     int(seq_shared), ptr(link, optional=True), ptr(regions, torch.float32), K,
                                                     G, S, L, A, kn['hb_cutoff'], *(ptr(out[k]) for k in ('torsion', 'have', 'bond', 'rama', 'ss', 'state',
                                                                                                          'partner', 'count')), stream()))
    return out


_RAMA_DEFAULT = {}


def _rama_default(device):
    """rama_regions() on `device`, cached per device: treat it as read-only"""
    key = str(torch.device(device))
    if key not in _RAMA_DEFAULT:
        _RAMA_DEFAULT[key] = rama_regions().to(device)
    return _RAMA_DEFAULT[key]


SIMILARITY_MAX_LEN = 256    # elements of a row of align_sequences / gapped_rmsd
SIMILARITY_MAX_TABLE = 32   # rows of a substitution table


def check_gaps(name, gap_open, gap_extend):
    """(int(gap_open), int(gap_extend)), or ValueError unless both are integers with -32767 <= gap_open <= gap_extend <= 0 (the check abopt_align_sequences
    makes, ahead of any device work; the alignment's statement equals the enumeration of all alignments only with gap_open <= gap_extend)."""
    for what, v in (('gap_open', gap_open), ('gap_extend', gap_extend)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f'{name}: {what} must be an integer (got {v!r}); scale the table and the gaps together, e.g. by 2 for halves')
    o, e = int(gap_open), int(gap_extend)
    if not -32767 <= o <= e <= 0:
        raise ValueError(f'{name}: expected -32767 <= gap_open <= gap_extend <= 0 (got gap_open={o}, gap_extend={e})')
    return o, e


def _similarity_rows(name, what, t, mask, floating):
    """One side of a similarity call, checked without a device: t (rows, n) integer, or (rows, n, 3) floating point with `floating`; 1 <= n <= 256; mask None or
    (rows, n).  -> (rows, n), or ValueError."""
    want = 3 if floating else 2
    kind = 'floating point (rows, n, 3)' if floating else 'integer (rows, n)'
    ok = t.dim() == want and (not floating or t.shape[2] == 3) and (t.dtype.is_floating_point if floating else not (t.dtype.is_floating_point or t.dtype.is_complex))
    if not ok:
        raise ValueError(f'{name}: {what} {tuple(t.shape)} {t.dtype} must be {kind}')
    rows, n = t.shape[0], t.shape[1]
    if not 1 <= n <= SIMILARITY_MAX_LEN:
        raise ValueError(f'{name}: {what} has {n} elements per row, expected 1 .. {SIMILARITY_MAX_LEN}')
    if mask is not None and tuple(mask.shape) != (rows, n):
        raise ValueError(f'{name}: the mask of {what} {tuple(mask.shape)} must be (rows, n) = {(rows, n)}')
    return rows, n


def _similarity_device(name, q, r):
    """Both sides on one HIP device, or ValueError: the last refusal, before anything is allocated."""
    if not (q.is_cuda and r.is_cuda):
        raise ValueError(f'{name}: the kernels run on a HIP device only; got a CPU tensor (there is no CPU path)')
    if q.device != r.device:
        raise ValueError(f'{name}: queries on {q.device} and references on {r.device} must share a device')
    ptr(q, strided=True)                                             # the current device is the tensors'
    return q.device


def _bytes(t):
    """integer residue types as contiguous uint8, clamped into 0..255 on the device like _seq_bytes"""
    return (t if t.dtype == torch.uint8 else t.to(torch.uint8) if t.dtype == torch.bool else t.clamp(0, 255).to(torch.uint8)).contiguous()


def align_sequences(q, r, table, gap_open, gap_extend, qmask=None, rmask=None):
    """Global alignment of every query row with every reference row: substitution table, affine gaps, end gaps free (include/abopt.h: abopt_align_sequences;
    DESIGN.md section 6.11).  q (Q, na) and r (R, nb), any integer dtype (clamped into 0..255), na, nb <= 256; qmask / rmask (optional, (Q, na) / (R, nb) bool):
    a row's sequence is its mask-true bytes in order, None = all; table (T, T) integer, 1 <= T <= 32, row = the query's byte, a byte >= T reads row or column
    T - 1, entries within +-32767 (`model.identity_table`, `model.substitution_table`); gap_open <= gap_extend <= 0, integers: a gap run of k columns inside
    the alignment costs gap_open + (k - 1) gap_extend, one that touches either end nothing.
    -> dict of device tensors (Q, R) int32: score (the maximum), matches (the most among the alignments of that score), columns (the fewest among those);
    100 matches / columns is the reference's seqid, up to its choice among co-optimal alignments.  One stream-ordered launch, no host synchronisation,
    capturable."""
    name = 'align_sequences'
    Q, na = _similarity_rows(name, 'q', q, qmask, False)
    R, nb = _similarity_rows(name, 'r', r, rmask, False)
    if table.dim() != 2 or table.shape[0] != table.shape[1] or not 1 <= table.shape[0] <= SIMILARITY_MAX_TABLE or table.dtype.is_floating_point or \
            table.dtype.is_complex:
        raise ValueError(f'{name}: table {tuple(table.shape)} {table.dtype} must be integer of shape (T, T), 1 <= T <= {SIMILARITY_MAX_TABLE}')
    o, e = check_gaps(name, gap_open, gap_extend)
    if Q * R > 0x7fffffff:
        raise ValueError(f'{name}: {Q} x {R} pairs exceed 2^31 - 1')
    dev = _similarity_device(name, q, r)
    q, r, qmask, rmask = _bytes(q), _bytes(r), _as_flags(qmask), _as_flags(rmask)
    table = table.to(device=dev, dtype=torch.int32).contiguous()
    new = torch.empty if Q * R else torch.zeros                      # an empty call launches nothing
    out = {k: new(Q, R, dtype=torch.int32, device=dev) for k in ('score', 'matches', 'columns')}
    _check(lib().abopt_align_sequences(ptr(q, torch.uint8), ptr(qmask, optional=True), ptr(r, torch.uint8), ptr(rmask, optional=True), ptr(table, torch.int32),
                                       table.shape[0], o, e, Q, R, na, nb, ptr(out['score']), ptr(out['matches']), ptr(out['columns']), stream()))
    return out


def gapped_rmsd(qca, rca, qmask=None, rmask=None):
    """The reference's gapped CA RMSD (tools/eval/similarity.py: reslist_rmsd) of every query row against every reference row, without superposition
    (include/abopt.h: abopt_gapped_rmsd).  qca (Q, na, 3) and rca (R, nb, 3) floating point, na, nb <= 256; qmask / rmask (optional,
    (Q, na) / (R, nb) bool): a row's residues are its mask-true ones in order, None = all.  The shorter list is placed in the longer, order kept, its last two
    residues adjacent (the reference's boundary), and the sum of squared CA deviations is minimised.
    -> dict of device tensors (Q, R): sd fp32 (the minimum; -1 if either side is empty), m int32 (the shorter length; 0 then), rmsd fp32 = sqrt(sd / m), -1
    where m is 0.  One launch and a few torch operations, stream-ordered, no host synchronisation, capturable."""
    name = 'gapped_rmsd'
    Q, na = _similarity_rows(name, 'qca', qca, qmask, True)
    R, nb = _similarity_rows(name, 'rca', rca, rmask, True)
    if Q * R > 0x7fffffff:
        raise ValueError(f'{name}: {Q} x {R} pairs exceed 2^31 - 1')
    dev = _similarity_device(name, qca, rca)
    qca, rca, qmask, rmask = qca.float().contiguous(), rca.float().contiguous(), _as_flags(qmask), _as_flags(rmask)
    new = torch.empty if Q * R else torch.zeros                      # an empty call launches nothing
    sd = new(Q, R, dtype=torch.float32, device=dev)
    m = new(Q, R, dtype=torch.int32, device=dev)
    _check(lib().abopt_gapped_rmsd(ptr(qca, torch.float32), ptr(qmask, optional=True), ptr(rca, torch.float32), ptr(rmask, optional=True), Q, R, na, nb, ptr(sd),
                                   ptr(m), stream()))
    rmsd = torch.where(m > 0, torch.sqrt(sd / m.clamp(min=1).float()), torch.full_like(sd, -1.0))
    return dict(sd=sd, m=m, rmsd=rmsd)


def superposed_rmsd(q, r, qfit=None, rfit=None, qscore=None, rscore=None, want_transform=False):
    """RMSD after best-fit superposition of every query row onto every reference row (include/abopt.h: abopt_superposed_rmsd).
    q (Q, na, 3) and r (R, nb, 3) floating point, na, nb <= 256; qfit / rfit (optional, (Q, na) / (R, nb) bool): the points the rotation and translation are
    fitted on, None = all; qscore / rscore (optional): the points the deviation is measured on, None = that row's fit points.  Points pair by rank: the k-th
    true element of a query row with the k-th true element of a reference row.  The query is the mobile side; proper rotations only.
    -> dict of device tensors (Q, R): rmsd fp32, n_fit and n_score int32 [, rot (Q, R, 3, 3) and trans (Q, R, 3) fp32 with want_transform: r ~ rot q + trans].
    A pair whose fit counts or score counts differ, with fewer than 3 fit points or no score point is NOT scored: rmsd -1, n_fit = n_score = 0, rot the
    identity, trans 0.  One stream-ordered launch, no host synchronisation, capturable."""
    name = 'superposed_rmsd'
    Q, na = _similarity_rows(name, 'q', q, qfit, True)
    R, nb = _similarity_rows(name, 'r', r, rfit, True)
    for what, m, want in (('qscore', qscore, (Q, na)), ('rscore', rscore, (R, nb))):
        if m is not None and tuple(m.shape) != want:
            raise ValueError(f'{name}: {what} {tuple(m.shape)} must be (rows, n) = {want}')
    if Q * R > 0x7fffffff:
        raise ValueError(f'{name}: {Q} x {R} pairs exceed 2^31 - 1')
    dev = _similarity_device(name, q, r)
    q, r = q.float().contiguous(), r.float().contiguous()
    qfit, rfit, qscore, rscore = _as_flags(qfit), _as_flags(rfit), _as_flags(qscore), _as_flags(rscore)
    new = torch.empty if Q * R else torch.zeros                      # an empty call launches nothing
    out = dict(rmsd=new(Q, R, dtype=torch.float32, device=dev), n_fit=new(Q, R, dtype=torch.int32, device=dev), n_score=new(Q, R, dtype=torch.int32, device=dev))
    if want_transform:
        out.update(rot=new(Q, R, 3, 3, dtype=torch.float32, device=dev), trans=new(Q, R, 3, dtype=torch.float32, device=dev))
    _check(lib().abopt_superposed_rmsd(ptr(q, torch.float32), ptr(qfit, optional=True), ptr(qscore, optional=True), ptr(r, torch.float32), ptr(rfit, optional=True),
                                       ptr(rscore, optional=True), Q, R, na, nb, ptr(out['rmsd']), ptr(out['n_fit']), ptr(out['n_score']),
                                       ptr(out.get('rot'), optional=True), ptr(out.get('trans'), optional=True), stream()))
    return out


def _pair_list(name, pairs, Q, R):
    """The optional (P, 2) list of (query row, reference row), checked without a device -> the number of pairs of the call.  The VALUES are not read here (that
    would synchronise): the kernels treat a pair outside the panels as documented."""
    if pairs is None:
        if Q * R > 0x7fffffff:
            raise ValueError(f'{name}: {Q} x {R} pairs exceed 2^31 - 1')
        return Q * R
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype.is_floating_point or pairs.dtype.is_complex or pairs.dtype == torch.bool:
        raise ValueError(f'{name}: pairs {tuple(pairs.shape)} {pairs.dtype} must be integer of shape (P, 2): (query row, reference row)')
    if pairs.shape[0] > 0x7fffffff:
        raise ValueError(f'{name}: {pairs.shape[0]} pairs exceed 2^31 - 1')
    return pairs.shape[0]


def align_traceback(q, r, table, gap_open, gap_extend, qmask=None, rmask=None, pairs=None, want_ops=True, want_rmap=False):
    """THE alignment of chosen pairs of rows -- which element is paired with which (include/abopt.h: abopt_align_traceback).  The
    arguments of `align_sequences`, plus pairs (optional, (P, 2) integer: query row, reference row; None = all Q R pairs, row-major).  Among the alignments with
    the best (score, matches, -columns), the one that is least when read from its last column to its first, a pair before a query residue against a gap before
    a gap against a reference residue.
    -> dict of device tensors over the P pairs: score, matches, columns (P) int32, equal to `align_sequences`; qmap (P, na) int16: for element k of the query
    row the element of the reference row it is paired with, -1 if masked out, against a gap or in a free overhang [, ops (P, na + nb) uint8 with want_ops: 1 a
    pair, 2 a query residue against a gap, 3 a gap against a reference residue, 0 beyond `columns`; rmap (P, nb) int16 with want_rmap: the inverse of qmap].
    A pair outside the panels: 0, 0, 0, ops 0, maps -1.  Score everything with `align_sequences`, choose, and trace the chosen: the maps of 10^6 pairs of rows
    of 256 are 0.5 GB.  One stream-ordered launch, no host synchronisation, capturable."""
    name = 'align_traceback'
    Q, na = _similarity_rows(name, 'q', q, qmask, False)
    R, nb = _similarity_rows(name, 'r', r, rmask, False)
    if table.dim() != 2 or table.shape[0] != table.shape[1] or not 1 <= table.shape[0] <= SIMILARITY_MAX_TABLE or table.dtype.is_floating_point or \
            table.dtype.is_complex:
        raise ValueError(f'{name}: table {tuple(table.shape)} {table.dtype} must be integer of shape (T, T), 1 <= T <= {SIMILARITY_MAX_TABLE}')
    o, e = check_gaps(name, gap_open, gap_extend)
    P = _pair_list(name, pairs, Q, R)
    dev = _similarity_device(name, q, r)
    if pairs is not None and pairs.device != dev:
        raise ValueError(f'{name}: pairs on {pairs.device} must be on {dev}')
    q, r, qmask, rmask = _bytes(q), _bytes(r), _as_flags(qmask), _as_flags(rmask)
    table = table.to(device=dev, dtype=torch.int32).contiguous()
    plist = None if pairs is None else pairs.to(torch.int32).contiguous()
    new = torch.empty if P else torch.zeros                          # an empty call launches nothing
    out = {k: new(P, dtype=torch.int32, device=dev) for k in ('score', 'matches', 'columns')}
    out['qmap'] = new(P, na, dtype=torch.int16, device=dev)
    if want_ops:
        out['ops'] = new(P, na + nb, dtype=torch.uint8, device=dev)
    if want_rmap:
        out['rmap'] = new(P, nb, dtype=torch.int16, device=dev)
    if pairs is None or P:                                           # an empty list has no address: NULL would mean "all pairs"
        _check(lib().abopt_align_traceback(ptr(q, torch.uint8), ptr(qmask, optional=True), ptr(r, torch.uint8), ptr(rmask, optional=True), ptr(table, torch.int32),
                                           table.shape[0], o, e, ptr(plist, optional=True), P, Q, R, na, nb, ptr(out['score']), ptr(out['matches']),
                                           ptr(out['columns']), ptr(out.get('ops'), optional=True), ptr(out['qmap']), ptr(out.get('rmap'), optional=True), stream()))
    return out


def superposed_rmsd_mapped(q, r, qmap, pairs=None, qfit=None, rfit=None, qscore=None, rscore=None, want_transform=False):
    """`superposed_rmsd` on the pairs a map names, so that rows of different lengths superpose (include/abopt.h: abopt_superposed_rmsd_mapped; DESIGN.md section
    6.14).  q (Q, na, 3), r (R, nb, 3) floating point; qmap (P, na) integer: for pair p, element k of the query row is paired with element qmap[p, k] of the
    reference row, anything outside [0, nb) = unpaired (`align_traceback`'s qmap, or a caller's own pairing -- it need not be monotone); pairs (optional, (P, 2):
    query row, reference row; None = all Q R, row-major); qfit / rfit: a pair is fitted on iff both its elements are true (None = all); qscore / rscore: measured
    on likewise (None = that side's fit mask).
    -> dict of device tensors over the P pairs: rmsd fp32, n_fit, n_score int32 [, rot (P, 3, 3), trans (P, 3) with want_transform].  Fewer than 3 fit pairs, no
    score pair or a pair outside the panels: -1, 0, 0, the identity, 0.  Equal bit for bit to `superposed_rmsd` on the same pairs gathered into rows of equal
    count.  One stream-ordered launch, no host synchronisation, capturable."""
    name = 'superposed_rmsd_mapped'
    Q, na = _similarity_rows(name, 'q', q, qfit, True)
    R, nb = _similarity_rows(name, 'r', r, rfit, True)
    for what, m, want in (('qscore', qscore, (Q, na)), ('rscore', rscore, (R, nb))):
        if m is not None and tuple(m.shape) != want:
            raise ValueError(f'{name}: {what} {tuple(m.shape)} must be (rows, n) = {want}')
    P = _pair_list(name, pairs, Q, R)
    if qmap.dim() != 2 or tuple(qmap.shape) != (P, na) or qmap.dtype.is_floating_point or qmap.dtype.is_complex or qmap.dtype == torch.bool:
        raise ValueError(f'{name}: qmap {tuple(qmap.shape)} {qmap.dtype} must be integer of shape (P, na) = {(P, na)}')
    dev = _similarity_device(name, q, r)
    for what, t in (('qmap', qmap), ('pairs', pairs)):
        if t is not None and t.device != dev:
            raise ValueError(f'{name}: {what} on {t.device} must be on {dev}')
    q, r = q.float().contiguous(), r.float().contiguous()
    qmap = (qmap if qmap.dtype == torch.int16 else qmap.clamp(-1, SIMILARITY_MAX_LEN).to(torch.int16)).contiguous()
    plist = None if pairs is None else pairs.to(torch.int32).contiguous()
    qfit, rfit, qscore, rscore = _as_flags(qfit), _as_flags(rfit), _as_flags(qscore), _as_flags(rscore)
    new = torch.empty if P else torch.zeros                          # an empty call launches nothing
    out = dict(rmsd=new(P, dtype=torch.float32, device=dev), n_fit=new(P, dtype=torch.int32, device=dev), n_score=new(P, dtype=torch.int32, device=dev))
    if want_transform:
        out.update(rot=new(P, 3, 3, dtype=torch.float32, device=dev), trans=new(P, 3, dtype=torch.float32, device=dev))
    if pairs is None or P:                                           # an empty list has no address: NULL would mean "all pairs"
        _check(lib().abopt_superposed_rmsd_mapped(ptr(q, torch.float32), ptr(r, torch.float32), ptr(qmap), ptr(plist, optional=True), P, ptr(qfit, optional=True),
                                                  ptr(qscore, optional=True), ptr(rfit, optional=True), ptr(rscore, optional=True), Q, R, na, nb, ptr(out['rmsd']),
                                                  ptr(out['n_fit']), ptr(out['n_score']), ptr(out.get('rot'), optional=True), ptr(out.get('trans'), optional=True),
                                                  stream()))
    return out


def check_lddt_cutoff(name, v):
    """float(v), or ValueError unless it is finite and > 0 (the check abopt_lddt_ca_grouped / abopt_lddt_ca_ensemble make on their cutoff, ahead of any device work)."""
    import math
    c = float(v)
    if not math.isfinite(c) or c <= 0.0:
        raise ValueError(f'{name} must be finite and > 0 (got {v!r})')
    return c


def lddt_ratio(num, den):
    """num / (4 den) in float64, rounded to fp32 once; -1 where den == 0 (the reference's lddt() returns eps / eps = 1.0 there: DESIGN.md section 6.5).  Pure torch,
    no host read."""
    d = den.double()
    return torch.where(den > 0, num.double() / (4.0 * d.clamp_min(1.0)), -1.0).float()


def _lddt_args(name, pos, mask, G, rows, group, cutoff):
    """Shape checks shared by the two lDDT calls (no device work) -> (S, L, A, shared, cutoff)."""
    if pos.dim() != 4 or mask.dim() != 3 or pos.shape[3] != 3:
        raise ValueError(f'{name}: expected pos (G*S, L, A, 3) and mask (G*S or G, L, A), got {tuple(pos.shape)} and {tuple(mask.shape)}')
    N, L, A = pos.shape[:3]
    if L < 1 or L > 16384 or (N % G if G else N):
        raise ValueError(f'{name}: {tuple(pos.shape)} candidates are not whole groups of {G} with 1 <= L <= 16384')
    if not 2 <= A <= 15:
        raise ValueError(f'{name}: A={A} atoms per residue, expected 2 .. 15 (atom slot 1 is the CA)')
    S = N // G if G else 0
    shared = mask.shape[0] != N or S == 1
    if tuple(mask.shape) != ((G if shared else N), L, A):
        raise ValueError(f'{name}: mask {tuple(mask.shape)} is neither per candidate nor per group')
    for what, t in (('rows', rows), ('group', group)):
        if t is not None and tuple(t.shape) != (G, L):
            raise ValueError(f'{name}: {what} {tuple(t.shape)} must be (G, L) = {(G, L)}')
    return S, L, A, shared, check_lddt_cutoff(f'{name}: cutoff', cutoff)


def _lddt_tensors(pos, mask, rows, group):
    pos, mask = _contig(pos.float(), mask if mask.dtype in (torch.bool, torch.uint8) else mask.bool())
    rows = None if rows is None else (rows if rows.dtype in (torch.bool, torch.uint8) else rows != 0).contiguous()
    group = None if group is None else group.to(torch.int32).contiguous()
    return pos, mask, rows, group


def lddt_ca_grouped(pos, mask, ref_pos, ref_mask, rows=None, group=None, cutoff=15.0):
    """lDDT-CA of G*S candidates against the G references of their groups, per residue and pooled (include/abopt.h: abopt_lddt_ca_grouped).
    pos (G*S,L,A,3); mask (G*S,L,A), or (G,L,A) shared by the S candidates of a group; ref_pos (G,L,A,3), ref_mask (G,L,A); atom slot 1 is the CA.  rows
    (optional, (G,L) bool): the residues that are scored; group (optional, (G,L) int): the interface form, only pairs with one residue of side 1 and one of side 2
    count; cutoff in Angstrom on the reference's CA-CA distance.
    -> dict of device tensors: num, den (G*S,L) int32 (hits of the four thresholds, scored pairs), lddt_res (G*S,L) fp32 = num / (4 den) and lddt (G*S,) fp32 =
    sum num / (4 sum den), both computed in float64 and rounded once, -1 where den == 0.  Stream-ordered, no host synchronisation."""
    name = 'lddt_ca_grouped'
    if ref_pos.dim() != 4 or ref_mask.dim() != 3:
        raise ValueError(f'{name}: expected ref_pos (G, L, A, 3) and ref_mask (G, L, A), got {tuple(ref_pos.shape)} and {tuple(ref_mask.shape)}')
    G = ref_pos.shape[0]
    S, L, A, shared, cut = _lddt_args(name, pos, mask, G, rows, group, cutoff)
    if tuple(ref_pos.shape) != (G, L, A, 3) or tuple(ref_mask.shape) != (G, L, A):
        raise ValueError(f'{name}: ref_pos {tuple(ref_pos.shape)} / ref_mask {tuple(ref_mask.shape)} do not match the candidates {tuple(pos.shape)}')
    ptr(pos, strided=True)                                          # a CPU tensor is refused here, before anything is allocated
    ptr(ref_pos, strided=True)
    pos, mask, rows, group = _lddt_tensors(pos, mask, rows, group)
    ref_pos, ref_mask, _, _ = _lddt_tensors(ref_pos, ref_mask, None, None)
    dev = pos.device
    num, den = torch.empty(G * S, L, dtype=torch.int32, device=dev), torch.empty(G * S, L, dtype=torch.int32, device=dev)
    buf = Workspace.get(max(16, lib().abopt_lddt_ws_bytes(G, S, L)), dev)
    _check(lib().abopt_lddt_ca_grouped(ptr(pos, torch.float32), ptr(mask), int(shared), ptr(ref_pos, torch.float32), ptr(ref_mask), ptr(rows, optional=True),
                                       ptr(group, torch.int32, optional=True), G, S, L, A, cut, ptr(num), ptr(den), ptr(buf), buf.numel(), stream()))
    return dict(num=num, den=den, lddt_res=lddt_ratio(num, den), lddt=lddt_ratio(num.sum(1, dtype=torch.int64), den.sum(1, dtype=torch.int64)))


def lddt_ca_ensemble(pos, mask, group_size, rows=None, group=None, cutoff=15.0):
    """lDDT-CA of every candidate of a group against every other one, pooled over the residues (include/abopt.h: abopt_lddt_ca_ensemble).
    pos (G*S,L,A,3) with S = group_size; mask (G*S,L,A) or (G,L,A); rows, group, cutoff as for lddt_ca_grouped.
    -> dict of device tensors: num, den (G,S,S) int32, entry (g, a, b) = candidate a as the reference, b as the model; lddt (G,S,S) fp32 = num / (4 den), -1 where
    den == 0 (the diagonal is 1 wherever it has a scored pair); consistency (G,S) fp32: for candidate b the mean of lddt(a, b) over the a != b with den > 0 (in
    float64, rounded once), -1 if there is none.  Stream-ordered, no host synchronisation."""
    name = 'lddt_ca_ensemble'
    S = int(group_size)
    if S < 1 and pos.shape[0]:
        raise ValueError(f'{name}: group_size must be >= 1 (got {group_size!r})')
    if S > 16384:
        raise ValueError(f'{name}: group_size {S} exceeds the maximum of 16384')
    G = pos.shape[0] // S if S else 0
    if G * S != pos.shape[0]:
        raise ValueError(f'{name}: {tuple(pos.shape)} candidates are not whole groups of {S}')
    _, L, A, shared, cut = _lddt_args(name, pos, mask, G, rows, group, cutoff)
    if G * S * S > 2 ** 31 - 1:
        raise ValueError(f'{name}: G S S = {G * S * S} entries exceed 2^31 - 1')
    ptr(pos, strided=True)                                          # a CPU tensor is refused here, before anything is allocated
    pos, mask, rows, group = _lddt_tensors(pos, mask, rows, group)
    dev = pos.device
    num, den = torch.empty(G, S, S, dtype=torch.int32, device=dev), torch.empty(G, S, S, dtype=torch.int32, device=dev)
    buf = Workspace.get(max(16, lib().abopt_lddt_ws_bytes(G, S, L)), dev)
    _check(lib().abopt_lddt_ca_ensemble(ptr(pos, torch.float32), ptr(mask), int(shared), ptr(rows, optional=True), ptr(group, torch.int32, optional=True),
                                        G, S, L, A, cut, ptr(num), ptr(den), ptr(buf), buf.numel(), stream()))
    peer = (den > 0) & ~torch.eye(S, dtype=torch.bool, device=dev)
    ratio = torch.where(peer, num.double() / (4.0 * den.double().clamp_min(1.0)), 0.0)
    cnt = peer.sum(1)
    consistency = torch.where(cnt > 0, ratio.sum(1) / cnt.clamp_min(1), -1.0).float()
    return dict(num=num, den=den, lddt=lddt_ratio(num, den), consistency=consistency)


def pair_bias_cache_layers(w_pair_bias_list, pair_feat):
    """The cache from bare proj_pair_bias weights (training: built once per step for all blocks) -> list of per-layer views."""
    n = len(w_pair_bias_list)
    ws = _contig(*[w.detach().float() for w in w_pair_bias_list])
    arr = (GaWeights * n)()
    for i, w in enumerate(ws):
        arr[i].w_pair_bias = ptr(w, torch.float32)
    cache = pair_bias_cache(arr, n, pair_feat)
    return list(cache.view(n, -1).unbind(0))


def ipa_core_train_forward(proj_local, R, t, z, mask, w_pair_bias, spatial_coef, pbc=None):
    """Training-mode IPA core: -> feat (N,L,1824), alpha head-major (N,12,L,L)  (include/abopt.h: abopt_ipa_core_train_forward)."""
    N, L = mask.shape
    dev = z.device
    feat = torch.empty(N, L, 1824, device=dev)
    alpha = torch.empty(N, 12, L, L, device=dev)
    nb = lib().abopt_ipa_train_workspace_bytes(N, L)
    buf = Workspace.get(nb, dev)
    proj_local, R, t, z, mask, w_pair_bias, spatial_coef = _contig(proj_local, R, t, z, mask, w_pair_bias, spatial_coef)
    _check(lib().abopt_ipa_core_train_forward(ptr(proj_local, torch.float32), ptr(R, torch.float32), ptr(t, torch.float32),
                                              ptr(z, torch.float32), ptr(mask, torch.bool),
                                              ptr(w_pair_bias, torch.float32), ptr(spatial_coef, torch.float32), ptr(pbc, torch.float32, optional=True),
                                              ptr(feat), ptr(alpha), N, L, z.shape[-1], ptr(buf), buf.numel(), stream()))
    return feat, alpha


def ipa_points_backward(dfeat, feat, R, t):
    """-> dout_cat (N,12,L,56) = [d feat_node | d aggregated points] head-major, delta (N,L,12)  (abopt_ipa_points_backward)."""
    N, L = feat.shape[:2]
    dout_cat = torch.empty(N, 12, L, 56, device=feat.device)
    delta = torch.empty(N, L, 12, device=feat.device)
    dfeat, feat, R, t = _contig(dfeat, feat, R, t)
    _check(lib().abopt_ipa_points_backward(ptr(dfeat, torch.float32), dfeat.shape[-1], ptr(feat, torch.float32),
                                           ptr(R, torch.float32), ptr(t, torch.float32), ptr(dout_cat), ptr(delta), N, L, stream()))
    return dout_cat, delta


def ipa_backward_operands(proj_local, R, t):
    """-> Aq, Ak (N,12,L,57), Av (N,12,L,56): head-major GEMM operands of the IPA backward (abopt_ipa_backward_operands)."""
    N, L = proj_local.shape[:2]
    dev = proj_local.device
    Aq, Ak, Av = torch.empty(N, 12, L, 57, device=dev), torch.empty(N, 12, L, 57, device=dev), torch.empty(N, 12, L, 56, device=dev)
    proj_local, R, t = _contig(proj_local, R, t)
    _check(lib().abopt_ipa_backward_operands(ptr(proj_local, torch.float32), ptr(R, torch.float32), ptr(t, torch.float32),
                                             ptr(Aq), ptr(Ak), ptr(Av), N, L, stream()))
    return Aq, Ak, Av


def ipa_backward_assemble(P1, P2, P3, Aq, Ak, R, spatial_coef):
    """-> d proj_local (N,L,2016), e (N,L,12) with e.sum((0, 1)) = d loss / d spatial_coef  (abopt_ipa_backward_assemble)."""
    N, _, L, _ = P1.shape
    dproj = torch.empty(N, L, 2016, device=P1.device)
    e = torch.empty(N, L, 12, device=P1.device)
    P1, P2, P3, R, spatial_coef = _contig(P1, P2, P3, R, spatial_coef)
    _check(lib().abopt_ipa_backward_assemble(ptr(P1, torch.float32), ptr(P2, torch.float32), ptr(P3, torch.float32),
                                             ptr(Aq, torch.float32), ptr(Ak, torch.float32), ptr(R, torch.float32),
                                             ptr(spatial_coef, torch.float32), ptr(dproj), ptr(e), N, L, stream()))
    return dproj, e


def ipa_pair_backward(z, alpha, dalpha_node, delta, dfeat, w_pair_bias, dz_into=None, want_dz=True, reduce=None):
    """alpha, dalpha_node head-major (N,12,L,L) -> g (N,12,L,L), dz (N,L,L,C), dWb (12,C)  (include/abopt.h: abopt_ipa_pair_backward).
    dz_into: an existing d pair_feat buffer this block's gradient is ADDED to (returned as dz).  want_dz=False: dz is None -- the caller
    assembles d pair_feat of all blocks at once (ipa_dz_assemble).  reduce: the column-sum function for the per-row partials of dWb (default
    hip.colsum; training passes WgradGroup's, which rides in the grouped weight-gradient launch)."""
    N, L = z.shape[:2]
    g = torch.empty_like(alpha)
    dz = None if not want_dz else (torch.empty_like(z) if dz_into is None else dz_into)
    dwb_rows = torch.empty(N * L, 12 * z.shape[-1], device=z.device)
    z, alpha, dalpha_node, delta, dfeat, w_pair_bias = _contig(z, alpha, dalpha_node, delta, dfeat, w_pair_bias)
    _check(lib().abopt_ipa_pair_backward(ptr(z, torch.float32), ptr(alpha, torch.float32), ptr(dalpha_node, torch.float32),
                                         ptr(delta, torch.float32), ptr(dfeat, torch.float32), dfeat.shape[-1],
                                         ptr(w_pair_bias, torch.float32), ptr(g), ptr(dz, torch.float32, optional=True), ptr(dwb_rows), int(dz_into is not None), N, L, z.shape[-1], stream()))
    return g, dz, (reduce or colsum)(dwb_rows).view(12, z.shape[-1])


def ipa_dz_assemble(alphas, gs, dfeats, wbs, like):
    """d pair_feat (shape of `like`) of all blocks of an encoder from their (alpha, g, d feat, proj_pair_bias.weight): abopt_ipa_dz_assemble."""
    nl = len(alphas)
    N, L, _, Cd = like.shape
    keep = [_contig(*ts) for ts in (alphas, gs, dfeats, [w.detach().float() for w in wbs])]
    ld = keep[2][0].shape[-1]
    assert all(t.shape[-1] == ld for t in keep[2])
    arr = lambda ts: (C.c_void_p * nl)(*[ptr(t, torch.float32).value for t in ts])
    dz = torch.empty_like(like)
    _check(lib().abopt_ipa_dz_assemble(nl, arr(keep[0]), arr(keep[1]), arr(keep[2]), ld, arr(keep[3]), ptr(dz), N, L, Cd, stream()))
    return dz


def encode_inputs(aa, res_nb, chain_nb, pos_atoms, mask_atoms, atoms, fragment_type=None, hotspot=None, structure_mask=None, sequence_mask=None):
    """-> (EncodeInputs, keepalive list).  Tensors are made contiguous; the struct only borrows their pointers."""
    N, L = aa.shape
    keep = [aa.contiguous(), res_nb.contiguous(), chain_nb.contiguous(), pos_atoms.contiguous(), mask_atoms.contiguous()]
    opt = [None if t is None else t.contiguous() for t in (fragment_type, hotspot, structure_mask, sequence_mask)]
    s = EncodeInputs(N, L, pos_atoms.shape[2], atoms, ptr(keep[0], torch.int64), ptr(keep[1], torch.int64), ptr(keep[2], torch.int64),
                     ptr(opt[0], torch.int64, optional=True), ptr(opt[1], torch.int64, optional=True), ptr(keep[3], torch.float32),
                     ptr(keep[4], torch.bool), ptr(opt[2], torch.bool, optional=True), ptr(opt[3], torch.bool, optional=True))
    return s, keep + opt


def residue_embed_forward(inp, weights, has_hotspot):
    N, L = inp.N, inp.L
    dev = torch.device('cuda', torch.cuda.current_device())
    res_feat = torch.empty(N, L, 128, device=dev)
    R = torch.empty(N, L, 3, 3, device=dev)
    p = torch.empty(N, L, 3, device=dev)
    nb = lib().abopt_residue_embed_workspace_bytes(N, L, inp.atoms, int(has_hotspot))
    buf = Workspace.get(nb, dev)
    _check(lib().abopt_residue_embed_forward(C.byref(inp), C.byref(weights), ptr(res_feat), ptr(R), ptr(p), ptr(buf), buf.numel(), stream()))
    return res_feat, R, p


PAIR_ACT = 288


def residue_features(inp, weights, in_dim):
    """-> features (N*L, in_dim) (a view of a buffer whose rows are padded to a multiple of 4 floats), R (N,L,3,3), p (N,L,3):
    abopt_residue_features, the inputs of ResidueEmbedding's MLP (residue.py:33-88)."""
    N, L = inp.N, inp.L
    dev = torch.device('cuda', torch.cuda.current_device())
    ld = (in_dim + 3) & ~3
    feat = torch.empty(N * L, ld, device=dev)
    R, p = torch.empty(N, L, 3, 3, device=dev), torch.empty(N, L, 3, device=dev)
    nb = lib().abopt_residue_features_workspace_bytes(N, L)
    buf = Workspace.get(nb, dev)
    _check(lib().abopt_residue_features(C.byref(inp), C.byref(weights), ptr(feat), ptr(R), ptr(p), ptr(buf), buf.numel(), stream()))
    return feat[:, :in_dim], R, p


def pair_embed_forward(inp, weights, save_activations=False, save_T=False):
    """-> pair_feat (N,L,L,64) [, activations (N,L,L,288), G, T (N,L,L,atoms*16) for the training backward; T is None unless save_T:
    the backward recomputes it from the atoms]."""
    N, L = inp.N, inp.L
    dev = torch.device('cuda', torch.cuda.current_device())
    pair_feat = torch.empty(N, L, L, 64, device=dev)
    acts = G = T = None
    if save_activations:
        acts = torch.empty(N, L, L, PAIR_ACT, device=dev)
        G = torch.empty(N, L, L, inp.atoms * 16, device=dev)
        T = torch.empty(N, L, L, inp.atoms * 16, device=dev) if save_T else None
    nb = lib().abopt_pair_embed_workspace_bytes(N, L, inp.atoms)
    buf = Workspace.get(nb, dev)
    _check(lib().abopt_pair_embed_forward(C.byref(inp), C.byref(weights), ptr(pair_feat), ptr(acts, optional=True), ptr(G, optional=True),
                                          ptr(T, optional=True), ptr(buf), buf.numel(), stream()))
    return (pair_feat, acts, G, T) if save_activations else pair_feat


PAIR_DY = 320


def pair_embed_backward(inp, weights, dpair_feat, acts, T=None, colsum=False):
    """-> dys (N,L,L,320), ds (N,L,L,atoms*16) [, column sums of dys (320) when colsum]  (include/abopt.h: abopt_pair_embed_backward).
    T None: recomputed in the kernel."""
    N, L = inp.N, inp.L
    dev = acts.device
    dys = torch.empty(N, L, L, PAIR_DY, device=dev)
    ds = torch.empty(N, L, L, inp.atoms * 16, device=dev)
    db = torch.empty(PAIR_DY, device=dev) if colsum else None
    nb = lib().abopt_pair_embed_backward_workspace_bytes(N, L, inp.atoms)
    buf = Workspace.get(nb, dev)
    dpair_feat, = _contig(dpair_feat)
    _check(lib().abopt_pair_embed_backward(C.byref(inp), C.byref(weights), ptr(dpair_feat, torch.float32), ptr(acts, torch.float32),
                                           ptr(T, torch.float32, optional=True), ptr(dys), ptr(ds), ptr(db, optional=True), ptr(buf), buf.numel(), stream()))
    return (dys, ds, db) if colsum else (dys, ds)


_BB_TABLES = {}


def reconstruct_backbone_partially(pos_ctx, R_new, t_new, aa, chain_nb, res_nb, mask_atoms, mask_recons):
    """geometry.py:404-480 on the device -> (pos_new (N,L,A,3), mask_new (N,L,A) bool)."""
    dev = pos_ctx.device
    if dev not in _BB_TABLES:
        import numpy as np
        d = np.load(os.path.join(_HERE, 'data', 'backbone_ideal.npz'))
        _BB_TABLES[dev] = (torch.from_numpy(d['bb_table']).to(dev).contiguous(), torch.from_numpy(d['o_table']).to(dev).contiguous())
    bb, ot = _BB_TABLES[dev]
    N, L, A = mask_atoms.shape
    pos_new = torch.empty(N, L, A, 3, device=dev)
    mask_new = torch.empty(N, L, A, dtype=torch.bool, device=dev)
    pos_ctx, R_new, t_new, aa, chain_nb, res_nb, mask_atoms, mask_recons = _contig(pos_ctx, R_new, t_new, aa, chain_nb, res_nb, mask_atoms, mask_recons)
    _check(lib().abopt_reconstruct_backbone_partially(ptr(pos_ctx, torch.float32), ptr(R_new, torch.float32),
                                                      ptr(t_new, torch.float32), ptr(aa, torch.int64),
                                                      ptr(chain_nb, torch.int64), ptr(res_nb, torch.int64),
                                                      ptr(mask_atoms, torch.bool), ptr(mask_recons, torch.bool),
                                                      ptr(bb), ptr(ot), ptr(pos_new), ptr(mask_new), N, L, A, stream()))
    return pos_new, mask_new


def _dockq_args(name, model_pos, model_mask, native_pos, native_mask, group):
    """The shape contract of hip.dockq_lite_grouped (hip.dockq_lite checks the same with G = 1, in its own words), checked without a device: the candidate side is _candidate_args (model_pos (G*S, L, A, 3) in whole groups of
    the G rows of group (G, L), model_mask (G*S, L, A) or (G, L, A)); the native side is native_pos (G, L, A, 3) and native_mask (G, L, A) with G >= 1; the CA
    is atom slot 1, so A >= 2.  -> (G, S, L, A, shared: the mask is per native), or ValueError."""
    G, S, L, A, shared = _candidate_args(name, model_pos, model_mask, group)
    if G < 1 or tuple(native_pos.shape) != (G, L, A, 3) or tuple(native_mask.shape) != (G, L, A):
        raise ValueError(f'{name}: native_pos {tuple(native_pos.shape)} and native_mask {tuple(native_mask.shape)} are not (G, L, A, 3) and (G, L, A) '
                         f'with G >= 1 for the (G, L, A) = {(G, L, A)} of the candidates and group')
    if A < 2:
        raise ValueError(f'{name}: A={A} atoms per residue, expected 2 .. 15 (the CA is atom slot 1)')
    return G, S, L, A, shared


def dockq_lite(model_pos, model_mask, native_pos, native_mask, group, check=True):
    """DockQ of S candidates against one native (include/abopt.h: abopt_dockq_lite) -> (S, 4) = fnat, irms, Lrms, DockQ.
    model_pos (S,L,A,3); model_mask (S,L,A) or (L,A) shared; native_pos (L,A,3); native_mask (L,A); group (L,) int {0,1,2}.
    check=True (one device read-back) raises, like the reference's asserts (DockQ.py:150-188), when a candidate has no CA atom
    common to model and native in its interface, receptor or ligand; check=False leaves the kernel's -1 markers in place.
    A wrong shape of any of the five tensors is a ValueError before any device call: what _dockq_args checks, with G = 1 and the shapes named as given;
    2 <= A <= 15; a three-dimensional model_mask has one row per candidate (a (1,L,A) mask with S > 1 is refused, not taken as shared)."""
    name = 'dockq_lite'
    shapes = [tuple(t.shape) for t in (model_pos, model_mask, native_pos, native_mask, group)]
    if [len(s) for s in shapes] not in ([4, 3, 3, 2, 1], [4, 2, 3, 2, 1]):
        raise ValueError(f'{name}: expected model_pos (S, L, A, 3), model_mask (S, L, A) or (L, A), native_pos (L, A, 3), native_mask (L, A) and group (L,), got '
                         f'{shapes[0]}, {shapes[1]}, {shapes[2]}, {shapes[3]} and {shapes[4]}')
    S, A, L = shapes[0][0], shapes[0][2], shapes[4][0]
    if L < 1 or shapes[0][1:] != (L, A, 3):
        raise ValueError(f'{name}: model_pos {shapes[0]} is not (S, L, A, 3) with the L = {L} of group {shapes[4]}')
    if not 2 <= A <= 15:
        raise ValueError(f'{name}: A={A} atoms per residue, expected 2 .. 15 (the CA is atom slot 1)')
    shared = len(shapes[1]) == 2
    if shapes[1] != ((L, A) if shared else (S, L, A)):
        raise ValueError(f'{name}: model_mask {shapes[1]} is neither per candidate {(S, L, A)} nor shared {(L, A)}')
    if shapes[2] != (L, A, 3) or shapes[3] != (L, A):
        raise ValueError(f'{name}: native_pos {shapes[2]} and native_mask {shapes[3]} are not {(L, A, 3)} and {(L, A)}')
    ptr(model_pos, strided=True)                                       # a CPU tensor is refused before anything is allocated
    model_pos, model_mask, native_pos, native_mask = _contig(model_pos.float(), model_mask, native_pos.float(), native_mask)
    group = group.to(torch.int32).contiguous()
    out = torch.empty(S, 4, dtype=torch.float32, device=model_pos.device)
    nb = lib().abopt_dockq_workspace_bytes(L)
    buf = Workspace.get(nb, model_pos.device)
    _check(lib().abopt_dockq_lite(ptr(model_pos, torch.float32), ptr(model_mask, torch.bool), int(shared), ptr(native_pos, torch.float32),
                                  ptr(native_mask, torch.bool), ptr(group, torch.int32), S, L, A, ptr(out), ptr(buf), buf.numel(), stream()))
    if check and S > 0 and bool((out[:, 1:3] < 0).any()):
        bad = (out[:, 1:3] < 0).any(1).nonzero().flatten().tolist()
        raise ValueError(f'dockq_lite: candidates {bad} have an empty interface / receptor / ligand CA selection (no atoms in both model and native)')
    return out


def dockq_lite_grouped(model_pos, model_mask, native_pos, native_mask, group, check=True):
    """DockQ of G*S candidates against G natives in one launch (include/abopt.h: abopt_dockq_lite_grouped) -> (G*S, 4) = fnat, irms, Lrms, DockQ;
    candidate c is scored against native c // S, and every row equals dockq_lite on its group alone, bit for bit.
    model_pos (G*S,L,A,3); model_mask (G*S,L,A), or (G,L,A) shared by the S candidates of a native; native_pos (G,L,A,3); native_mask (G,L,A);
    group (G,L) int {0,1,2}.  check: as dockq_lite.  A wrong shape of any of the five tensors is a ValueError before any device call (_dockq_args)."""
    G, S, L, A, shared = _dockq_args('dockq_lite_grouped', model_pos, model_mask, native_pos, native_mask, group)
    N = G * S
    ptr(model_pos, strided=True)                                       # a CPU tensor is refused before anything is allocated
    model_pos, model_mask, native_pos, native_mask = _contig(model_pos.float(), model_mask, native_pos.float(), native_mask)
    group = group.to(torch.int32).contiguous()
    out = torch.empty(N, 4, dtype=torch.float32, device=model_pos.device)
    nb = lib().abopt_dockq_grouped_workspace_bytes(G, L)
    buf = Workspace.get(nb, model_pos.device)
    _check(lib().abopt_dockq_lite_grouped(ptr(model_pos, torch.float32), ptr(model_mask, torch.bool), int(shared), ptr(native_pos, torch.float32),
                                          ptr(native_mask, torch.bool), ptr(group, torch.int32), G, S, L, A, ptr(out), ptr(buf), buf.numel(), stream()))
    if check and N > 0 and bool((out[:, 1:3] < 0).any()):
        bad = (out[:, 1:3] < 0).any(1).nonzero().flatten().tolist()
        raise ValueError(f'dockq_lite_grouped: candidates {bad} have an empty interface / receptor / ligand CA selection (no atoms in both model and native)')
    return out


def pack_tail_weights(w_out, w0, w1, w2, transposed=False):
    """(w_out_frag, w_mlp_frag[, w_mlpT_frag]) packed on the device in one launch (include/abopt.h: abopt_pack_tail_weights)."""
    dev = w_out.device
    w_out, w0, w1, w2 = _contig(w_out.detach().float(), w0.detach().float(), w1.detach().float(), w2.detach().float())
    wof = torch.empty(lib().abopt_out_frag_floats(), dtype=torch.float32, device=dev)
    wmf = torch.empty(lib().abopt_mlp_frag_floats(), dtype=torch.float32, device=dev)
    wmt = torch.empty(lib().abopt_mlp_frag_floats(), dtype=torch.float32, device=dev) if transposed else None
    _check(lib().abopt_pack_tail_weights(ptr(w_out, torch.float32), ptr(w0, torch.float32), ptr(w1, torch.float32), ptr(w2, torch.float32),
                                         ptr(wof), ptr(wmf), ptr(wmt, torch.float32, optional=True), stream()))
    return (wof, wmf, wmt) if transposed else (wof, wmf)


def out_frag_terms(wof):
    """w_out_frag -> w_out_terms, what the fused core + tail kernel streams (abopt_out_frag_terms; since ABI 39 the two layouts are the same and
    this is a copy)."""
    wot = torch.empty(lib().abopt_out_terms_floats(), dtype=torch.float32, device=wof.device)
    _check(lib().abopt_out_frag_terms(ptr(wof, torch.float32), ptr(wot), stream()))
    return wot


def block_tail_forward(feat, wof, wmf, x, b_out, mask, g1, be1, b0, b1, b2, g2, be2, save=False):
    """out = LN2(y + MLP(y)), y = LN1(x + mask * (feat W_out^T + b_out)) for [rows, .] inputs (abopt_block_tail_forward).
    save=True also returns the [5, rows, 128] activation dump the backward consumes."""
    rows = x.numel() // 128
    feat, x, mask, b_out, g1, be1, b0, b1, b2, g2, be2 = _contig(feat, x, mask, b_out, g1, be1, b0, b1, b2, g2, be2)
    out = torch.empty_like(x)
    saved = torch.empty(5, rows, 128, dtype=torch.float32, device=x.device) if save else None
    f = lambda t: ptr(t, torch.float32)
    _check(lib().abopt_block_tail_forward(f(feat), f(wof), f(wmf), f(x), f(b_out), ptr(mask, torch.bool), f(g1), f(be1), f(b0), f(b1), f(b2), f(g2), f(be2),
                                          ptr(out), ptr(saved, torch.float32, optional=True), rows, stream()))
    return (out, saved) if save else out


def block_tail_backward(dout, saved, wmt, mask, g1, g2, reduce=None):
    """Row-local backward of the tail (abopt_block_tail_backward) -> dpre [3, rows, 128], da1, du [rows, 128], colsum [8, 128].
    reduce: the column-sum function for the per-workgroup partials (default hip.colsum; see ipa_pair_backward)."""
    rows = saved.shape[1]
    dout, mask, g1, g2 = _contig(dout, mask, g1, g2)
    dev = dout.device
    dpre = torch.empty(3, rows, 128, dtype=torch.float32, device=dev)
    da1 = torch.empty(rows, 128, dtype=torch.float32, device=dev)
    du = torch.empty(rows, 128, dtype=torch.float32, device=dev)
    colpart = torch.empty((rows + 31) // 32, 8, 128, dtype=torch.float32, device=dev)
    f = lambda t: ptr(t, torch.float32)
    _check(lib().abopt_block_tail_backward(f(dout), f(saved), f(wmt), ptr(mask, torch.bool), f(g1), f(g2), ptr(dpre), ptr(da1), ptr(du), ptr(colpart),
                                           rows, stream()))
    return dpre, da1, du, (reduce or colsum)(colpart.view(colpart.shape[0], -1)).view(8, 128)


def _operand(t):
    """(tensor, ld, batch stride, transposed) of a 2-D / 3-D fp32 operand whose matrices are row- or column-major; anything else is copied."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    b, r, c = t.shape
    sb, sr, sc_ = t.stride()
    if b == 1:
        sb = 0
    if sc_ == 1 and sr >= max(c, 1):
        return t, sr, sb, 0
    if sr == 1 and sc_ >= max(r, 1):
        return t, sc_, sb, 1
    t = t.contiguous()
    return t, t.stride(1), (t.stride(0) if b > 1 else 0), 0


def gemm(a, b, alpha=1.0, out=None, bias=None, relu=False):
    """C = alpha * a @ b^T on libabopt_hip.so (include/abopt.h: abopt_gemm).  a (M,K) or (B,M,K); b (N,K) or (B,N,K); either may be
    a transposed VIEW (x.t(), x.transpose(1, 2)): the kernel reads k-strided operands in place.  Batch broadcasting: a 2-D operand
    serves every batch.  bias (N,) and relu: y = relu(a b^T + bias) in the product's epilogue.  out (optional): (M,N) / (B,M,N) fp32 with
    unit column stride; it may be a column slice of a wider matrix (ldc = its row stride > N) -- the other columns are left untouched."""
    nb = max(a.shape[0] if a.dim() == 3 else 1, b.shape[0] if b.dim() == 3 else 1)
    a, lda, sa, at = _operand(a.float())
    b, ldb, sb, bt = _operand(b.float())
    M, K, N = a.shape[1], a.shape[2], b.shape[1]
    assert b.shape[2] == K, (a.shape, b.shape)
    c = torch.empty(nb, M, N, dtype=torch.float32, device=a.device) if out is None else out
    ldc, sc = N, M * N
    if out is not None:
        o3 = out if out.dim() == 3 else out.unsqueeze(0)
        if o3.shape != (nb, M, N) or o3.stride(2) != 1 or out.dtype != torch.float32 or not out.is_cuda:
            raise TypeError('gemm: out must be fp32 (B,M,N) on the device with unit column stride')
        ldc, sc = o3.stride(1), (o3.stride(0) if nb > 1 else 0)
    tiles = ((M + 63) // 64) * ((N + 63) // 64) * nb
    ws = None
    # split-K slabs: the C side (gemm.hip: launch_gemm_batched) splits below 256 output tiles, for a densely packed C only, into at most
    # min(1024 / tiles, K / 256) slabs -- size the workspace for exactly that (an env-tuned ABOPT_GEMM_TMAX / _KDIV build clamps to what it gets)
    dense_c = ldc == N and (nb == 1 or sc == M * N)
    if tiles < 256 and K >= 1024 and bias is None and not relu and dense_c:
        ws = Workspace.get(max(1, min(1024 // tiles, K // 256)) * nb * M * N * 4, a.device)
    if bias is not None:
        bias = bias.detach().float().contiguous()
        assert bias.numel() == N
    _check(lib().abopt_gemm(ptr(a, torch.float32, strided=True), lda, sa, at, ptr(b, torch.float32, strided=True), ldb, sb, bt, ptr(c, torch.float32, strided=True), ldc, sc, M, N, K, nb, float(alpha),
                            ptr(bias, torch.float32, optional=True), int(bool(relu)), ptr(ws, optional=True), ws.numel() if ws is not None else 0, stream()))
    return c


GEMM_TN_GROUP_MAX = 24


def gemm_tn_grouped(pairs, outs=None):
    """[a_p^T @ b_p for (a_p, b_p) in pairs] -- tall 2-D fp32 operands (K_p, M_p), (K_p, N_p) with unit column stride, column slices of wider
    matrices read in place -- as ONE product launch + ONE slab-sum launch per 24 pairs (include/abopt.h: abopt_gemm_tn_grouped): the
    weight-gradient products of a backward pass.  Returns the list of (M_p, N_p) results (`outs`: contiguous fp32 tensors to write, else fresh ones)."""
    res = []
    for i0 in range(0, len(pairs), GEMM_TN_GROUP_MAX):
        chunk = pairs[i0:i0 + GEMM_TN_GROUP_MAX]
        arr = (GemmTnProblem * len(chunk))()
        keep, tiles = [], 0
        for j, (q, (a, b)) in enumerate(zip(arr, chunk)):
            if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0] or a.stride(1) != 1 or b.stride(1) != 1 or a.shape[0] == 0:
                raise TypeError(f'gemm_tn_grouped: operands must be 2-D (K, M) / (K, N) with unit column stride and K > 0, got {tuple(a.shape)} {tuple(a.stride())} / {tuple(b.shape)} {tuple(b.stride())}')
            c = torch.empty(a.shape[1], b.shape[1], dtype=torch.float32, device=a.device) if outs is None else outs[i0 + j]
            if tuple(c.shape) != (a.shape[1], b.shape[1]):
                raise TypeError(f'gemm_tn_grouped: out {tuple(c.shape)} for operands {tuple(a.shape)} / {tuple(b.shape)}')
            q.a, q.b, q.c = ptr(a, torch.float32, strided=True), ptr(b, torch.float32, strided=True), ptr(c)
            q.lda, q.ldb, q.m, q.n, q.k = a.stride(0), b.stride(0), a.shape[1], b.shape[1], a.shape[0]
            tiles += ((q.m + 63) // 64) * ((q.n + 63) // 64)
            keep.append(c)
        want = max(1024 // tiles, 1) if tiles < 256 else 1
        need = sum(min(want, q.k // 256) * q.m * q.n for q in arr if min(want, q.k // 256) > 1)
        ws = Workspace.get(need * 4, chunk[0][0].device) if need else None
        _check(lib().abopt_gemm_tn_grouped(arr, len(chunk), ptr(ws, optional=True), ws.numel() if ws is not None else 0, stream()))
        res += keep
    return res


def colsum(x):
    """x.sum(0) for a 2-D fp32 tensor with unit column stride (a row-sliced / column-sliced view is read in place): abopt_colsum."""
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype != torch.float32 or not x.is_cuda or x.shape[0] == 0:
        return x.sum(0)
    rows, cols = x.shape
    out = torch.empty(cols, dtype=torch.float32, device=x.device)
    ws = Workspace.get(1024 * max(cols, 128) * 4, x.device)
    _check(lib().abopt_colsum(ptr(x, torch.float32, strided=True), x.stride(0), rows, cols, ptr(out), ptr(ws), ws.numel(), stream()))
    return out


def dpm_losses(R_pred, R_0, p_pred, p_target, c_den, s_t, s_0, abar_t, mask_generate):
    """-> sums (3,) of (rot, pos, seq) over the generated residues, and d(sum)/d(R_pred, p_pred, c_den) (abopt_dpm_losses)."""
    R_pred, R_0, p_pred, p_target, c_den, s_t, s_0, abar_t, mask_generate = _contig(R_pred.float(), R_0.float(), p_pred.float(), p_target.float(), c_den.float(),
                                                                                    s_t, s_0, abar_t.float(), mask_generate)
    N, L = mask_generate.shape
    nblk = (N * L + 255) // 256
    part = torch.empty(nblk, 3, dtype=torch.float32, device=R_pred.device)
    gR, gp, gc = torch.empty_like(R_pred), torch.empty_like(p_pred), torch.empty_like(c_den)
    _check(lib().abopt_dpm_losses(ptr(R_pred, torch.float32), ptr(R_0, torch.float32), ptr(p_pred, torch.float32), ptr(p_target, torch.float32), ptr(c_den, torch.float32),
                                  ptr(s_t, torch.int64), ptr(s_0, torch.int64), ptr(abar_t, torch.float32), ptr(mask_generate, torch.bool), N, L, ptr(part), ptr(gR), ptr(gp),
                                  ptr(gc), stream()))
    return colsum(part), gR, gp, gc


def abdock_losses(prmsd_logits, p_pred, p0n, coef_a, coef_b, mask_generate, mask_res, offsets, scale, pred_x0):
    """-> parts (N,4) = {CE_n, m0_n, smooth-l1 sum_n, count_n}, d prmsd_logits (N,nb) = softmax - onehot, d p_pred (N,L,3) of the smooth-l1 sum
    (abopt_abdock_losses: the prmsd and dist losses of the AbDock flavour, dpm_full.py:180-198,369-378)."""
    N, L = mask_generate.shape
    nb = prmsd_logits.shape[-1]
    prmsd_logits, p_pred, p0n, mask_generate, mask_res, offsets = _contig(prmsd_logits.float(), p_pred.float(), p0n.float(), mask_generate, mask_res, offsets.float())
    ca = cb = None
    if not pred_x0:
        ca, cb = _contig(coef_a.float(), coef_b.float())
    part = torch.empty(N, 4, dtype=torch.float32, device=p_pred.device)
    gl, gp = torch.empty_like(prmsd_logits), torch.empty_like(p_pred)
    _check(lib().abopt_abdock_losses(ptr(prmsd_logits, torch.float32), ptr(p_pred, torch.float32), ptr(p0n, torch.float32), ptr(ca, torch.float32, optional=True),
                                     ptr(cb, torch.float32, optional=True), ptr(mask_generate, torch.bool), ptr(mask_res, torch.bool), ptr(offsets, torch.float32), nb, N, L,
                                     float(scale), int(bool(pred_x0)), ptr(part), ptr(gl), ptr(gp), stream()))
    return part, gl, gp


def layer_norm_forward(x, gamma, beta, eps, save=True):
    """Rows of x (.., cols <= 256) through the reference's LayerNorm (layers.py:146-155) -> y [, xhat, rstd for the backward] (abopt_layer_norm_forward)."""
    cols = x.shape[-1]
    x2, gamma, beta = _contig(x.float().reshape(-1, cols), gamma.detach().float(), beta.detach().float())
    rows = x2.shape[0]
    y = torch.empty_like(x2)
    xhat = torch.empty_like(x2) if save else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x2.device) if save else None
    _check(lib().abopt_layer_norm_forward(ptr(x2, torch.float32), ptr(gamma, torch.float32), ptr(beta, torch.float32), cols, float(eps), rows, ptr(y),
                                          ptr(xhat, torch.float32, optional=True), ptr(rstd, torch.float32, optional=True), stream()))
    return y.view(x.shape), xhat, rstd


def layer_norm_backward(dy, xhat, rstd, gamma):
    """-> dx (shape of dy), d gamma, d beta (abopt_layer_norm_backward + two column sums)."""
    cols = dy.shape[-1]
    dy2, gamma = _contig(dy.float().reshape(-1, cols), gamma.detach().float())
    rows = dy2.shape[0]
    dx, dyx = torch.empty_like(dy2), torch.empty_like(dy2)
    _check(lib().abopt_layer_norm_backward(ptr(dy2, torch.float32), ptr(xhat, torch.float32), ptr(rstd, torch.float32), ptr(gamma, torch.float32), cols, rows,
                                           ptr(dx), ptr(dyx), stream()))
    return dx.view(dy.shape), colsum(dyx), colsum(dy2)


def heads_epilogue_forward(R, eps_crd, eps_rot, mask_generate):
    """-> R_next (.., 3, 3), eps_pos (.., 3): dpm_full.py:95-101 without the log map (abopt_heads_epilogue_forward)."""
    R, eps_crd, eps_rot, mask_generate = _contig(R.float(), eps_crd.float(), eps_rot.float(), mask_generate)
    rows = mask_generate.numel()
    R_next, eps_pos = torch.empty_like(R), torch.empty_like(eps_crd)
    _check(lib().abopt_heads_epilogue_forward(ptr(R, torch.float32), None, ptr(eps_crd, torch.float32), ptr(eps_rot, torch.float32), ptr(mask_generate, torch.bool),
                                              None, ptr(R_next), ptr(eps_pos), rows, 0, stream()))
    return R_next, eps_pos


def heads_epilogue_backward(R, eps_rot, mask_generate, dR_next, deps_pos):
    """-> d eps_crd, d eps_rot (.., 3) (abopt_heads_epilogue_backward); dR_next / deps_pos may be None (= zero)."""
    R, eps_rot, mask_generate = _contig(R.float(), eps_rot.float(), mask_generate)
    dR_next = None if dR_next is None else dR_next.float().contiguous()
    deps_pos = None if deps_pos is None else deps_pos.float().contiguous()
    rows = mask_generate.numel()
    d_crd, d_rot = torch.empty_like(eps_rot), torch.empty_like(eps_rot)
    _check(lib().abopt_heads_epilogue_backward(ptr(R, torch.float32), ptr(eps_rot, torch.float32), ptr(mask_generate, torch.bool), ptr(dR_next, torch.float32, optional=True),
                                               ptr(deps_pos, torch.float32, optional=True), ptr(d_crd), ptr(d_rot), rows, stream()))
    return d_crd, d_rot


def bucket_colsum(x, idx, buckets):
    """out[b] = sum of the rows of x (2-D fp32, unit column stride, read in place) whose idx is b; rows with idx < 0 are skipped."""
    rows, cols = x.shape
    if x.stride(1) != 1 or x.dtype != torch.float32 or not x.is_cuda or idx.dtype != torch.int32 or idx.numel() != rows:
        raise TypeError('bucket_colsum: fp32 [rows, cols] with unit column stride and an int32 index per row')
    out = torch.empty(buckets, cols, dtype=torch.float32, device=x.device)
    ws = Workspace.get(max(1, min(rows // 64, 2048 // ((cols + 63) // 64))) * buckets * cols * 4, x.device)      # the slices launch_bucket_colsum takes (gemm.hip)
    _check(lib().abopt_bucket_colsum(ptr(x, torch.float32, strided=True), x.stride(0), rows, cols, ptr(idx.contiguous(), torch.int32), buckets, ptr(out),
                                     ptr(ws), ws.numel(), stream()))
    return out


def segment_bucket_colsum(x, segments, idx, idx_div, buckets):
    """x (2-D fp32 [segments * rows_per_segment, cols], unit column stride, read in place) -> [segments, buckets, cols]: per segment, the rows
    summed by bucket; the bucket of row j of segment s is idx.flatten()[(s // idx_div) * rows_per_segment + j] (abopt_segment_bucket_colsum)."""
    rows, cols = x.shape
    rps = rows // segments
    if x.stride(1) != 1 or x.dtype != torch.float32 or not x.is_cuda or idx.dtype != torch.int32 or rps * segments != rows or idx.numel() * idx_div != rows:
        raise TypeError('segment_bucket_colsum: fp32 [segments * rows_per_segment, cols] with unit column stride and an int32 index row per idx_div segments')
    out = torch.empty(segments, buckets, cols, dtype=torch.float32, device=x.device)
    _check(lib().abopt_segment_bucket_colsum(ptr(x, torch.float32, strided=True), x.stride(0), segments, rps, cols, ptr(idx.contiguous(), torch.int32), idx_div, buckets,
                                             ptr(out), stream()))
    return out


def adam_step(params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay=0.0, max_grad_norm=None, grad_norm_out=None, ws=None,
              hyper_dev=None):
    """clip_grad_norm_ + torch.optim.Adam.step for a list of fp32 tensors in a handful of launches (abopt_adam_step; A/train.py:116-117).
    step: int64 device tensor of one element, incremented by the call.  grad_norm_out (1 float on the device) receives the unclipped norm
    when max_grad_norm is given.  The gradient tensors are read, not rewritten.  ws: the caller's scratch (adam_ws_bytes), else the shared one.
    hyper_dev: 6 float64 on the device {lr, beta1, beta2, eps, weight_decay, max_grad_norm}, read by the kernels instead of the scalars
    (graph replays follow a scheduler)."""
    n = len(params)
    if n == 0:
        return
    for group in (params, grads, exp_avg, exp_avg_sq):
        for t in group:
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise TypeError('adam_step: contiguous fp32 HIP tensors only')
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    numel = (C.c_int64 * n)(*[t.numel() for t in params])
    need = lib().abopt_adam_ws_floats(n, numel)
    if ws is None or ws.numel() * ws.element_size() < need * 4:
        ws = Workspace.get(need * 4, params[0].device)
    _check(lib().abopt_adam_step(n, arr(params), arr(grads), arr(exp_avg), arr(exp_avg_sq), numel, lr, beta1, beta2, eps, weight_decay,
                                 float(max_grad_norm) if max_grad_norm is not None else 0.0, ptr(step, torch.int64), ptr(ws), need,
                                 ptr(grad_norm_out, torch.float32, optional=True), ptr(hyper_dev, torch.float64, optional=True), stream()))


def adam_ws_bytes(params):
    n = len(params)
    return 4 * lib().abopt_adam_ws_floats(n, (C.c_int64 * n)(*[t.numel() for t in params])) if n else 0


def prof_enable(on=True):
    _check(lib().abopt_prof_enable(int(on)))


GRAPH_CAPTURE_EVENTS = False      # bench.py experiment: keep the IPA-core event records inside a captured loop graph
GRAPH_CAPTURE_SPANS = False       # bench.py: give the dominant kernel's launches span slots while a loop graph is captured (abopt_prof_spans)


def prof_spans_reset():
    _check(lib().abopt_prof_spans_reset(stream()))


def prof_spans():
    """(launches, total_ms) of the 32-row IPA launches that ran since prof_spans_reset(), from their in-kernel wall-clock spans."""
    n, ms = C.c_int(), C.c_double()
    _check(lib().abopt_prof_spans(C.byref(n), C.byref(ms)))
    return n.value, ms.value


def prof_clock():
    """(cycles, seconds, GHz) of wave 0 / workgroup 0 of the most recent 32-row IPA launch (abopt_prof_clock); None before any."""
    c, w = C.c_longlong(), C.c_longlong()
    _check(lib().abopt_prof_clock(C.byref(c), C.byref(w)))
    if w.value <= 0:
        return None
    return c.value, w.value * 1e-8, c.value / (w.value * 10.0)


def prof_collect(keep=False):
    """(launches, total_ms) of the IPA-core kernel since prof_enable(True).  keep=True: do not forget the event pairs (they were
    captured into a hipGraph and every replay records them again)."""
    n, ms = C.c_int(), C.c_double()
    _check((lib().abopt_prof_peek if keep else lib().abopt_prof_collect)(C.byref(n), C.byref(ms)))
    return n.value, ms.value
