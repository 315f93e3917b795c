"""ctypes binding of libidg_mi355x.so (the C ABI in include/idg_mi355x.h).

The library is built in-tree (`make -C ska-sdp-idg-bench_amd`, or
__graft_entry__.build()).  There is no fallback: if the library is missing
or fails to load, importing this module raises.
"""
import ctypes
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# IDG_MI355X_LIB selects another build of the same library (A/B-testing a
# kernel variant); it is read once, at import.
LIB_PATH = os.environ.get("IDG_MI355X_LIB") or os.path.join(
    PKG_DIR, "libidg_mi355x.so")

_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float
_Z = ctypes.c_size_t
_U64 = ctypes.c_uint64
_D = ctypes.c_double
_S = ctypes.c_char_p

# name -> (restype, argtypes); mirrors include/idg_mi355x.h one to one.
SIGNATURES = {
    "idg_abi_version": (_I, []),
    "idg_last_error": (_S, []),
    "idg_c_run_gridder": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _Z, _P, _P,
                               _P, _P, _Z, _P, _P]),
    "idg_c_run_degridder": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _Z, _P, _P,
                                 _P, _P, _Z, _P, _P]),
    "idg_gridder_launch": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _P, _P, _P,
                                _P, _P, _P, _P]),
    "idg_gridder_fft_launch": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _P, _P,
                                    _P, _P, _P, _P, _P]),
    "idg_degridder_launch": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _P, _P, _P,
                                  _P, _P, _P, _P]),
    "idg_validate_metadata": (_I, [_I, _I, _I, _I, _Z, _Z, _P]),
    "idg_host_chunk_plan": (_I, [_I, _P, _Z, _P, _I]),
    "idg_kernel_name": (_S, [_I, _I, _I]),
    "idg_precision_options": (_I, [_I, _I, _I]),
    "idg_p_run_gridder": (_D, []),
    "idg_p_run_degridder": (_D, []),
    "idg_print_device_info": (None, []),
    "idg_print_benchmark": (None, []),
    "idg_get_device_name": (_I, [ctypes.c_char_p, _Z]),
    "idg_flops_gridder": (_U64, [_U64, _U64, _U64, _U64, _U64]),
    "idg_bytes_gridder": (_U64, [_U64, _U64, _U64, _U64, _U64]),
    "idg_generate": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P,
                          _P, _I]),
    "idg_subgrid_fft_launch": (_I, [_I, _I, _I, _F, _P, _P]),
    "idg_adder_launch": (_I, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "idg_splitter_launch": (_I, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "idg_splitter_fft_launch": (_I, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "idg_release_workspaces": (_I, [_P, _I]),
    # the entries above plus a trailing const idg_options_t *
    "idg_c_run_gridder_opts": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _Z, _P,
                                    _P, _P, _P, _Z, _P, _P, _P]),
    "idg_c_run_degridder_opts": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _Z, _P,
                                      _P, _P, _P, _Z, _P, _P, _P]),
    "idg_gridder_launch_opts": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _P, _P,
                                     _P, _P, _P, _P, _P, _P]),
    "idg_gridder_fft_launch_opts": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _P,
                                         _P, _P, _P, _P, _P, _P, _P]),
    "idg_degridder_launch_opts": (_I, [_I, _I, _I, _F, _F, _I, _I, _P, _P, _P,
                                       _P, _P, _P, _P, _P, _P]),
    "idg_kernel_name_opts": (_S, [_I, _I, _I, _P]),
    "idg_precision_options_opts": (_I, [_I, _I, _I, _P]),
    "idg_auto_selected": (_I, [_I, _I, _P, _P, _P]),
    "idg_plan": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _I, _P, _I]),
    "idg_plan_launch": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P]),
    "idg_grid_fft_launch": (_I, [_I, _I, _I, _F, _P, _P]),
    "idg_grid_to_image_launch": (_I, [_I, _I, _F, _F, _P, _P, _P, _P]),
    "idg_image_to_grid_launch": (_I, [_I, _I, _F, _F, _P, _P, _P, _P]),
    "idg_taper_to_image": (_I, [_I, _I, _P, _P]),
    "idg_weight_density": (_I, [_P, _I, _I, _I, _P, _P, _Z, _P, _P, _P]),
    "idg_weight_density_launch": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _P,
                                       _P]),
    "idg_weight_scheme": (_I, [_P, _P, _P]),
    "idg_weight_scheme_launch": (_I, [_P, _P, _P, _P]),
    "idg_weight_apply": (_I, [_P, _I, _I, _P, _P, _Z, _P, _P, _P, _P, _P, _P,
                              _P, _P]),
    "idg_weight_apply_launch": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P,
                                     _P, _P, _P, _P]),
    "idg_clean": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "idg_clean_launch": (_I, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "idg_clark": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "idg_clark_launch": (_I, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "idg_beam_from_axes": (_I, [_D, _D, _D, _P]),
    "idg_beam_fit": (_I, [_I, _P, _F, _P]),
    "idg_beam_radius": (_I, [_P, _D]),
    "idg_beam_taps": (_I, [_P, _I, _P]),
    "idg_restore": (_I, [_P, _P, _P, _P, _P]),
    "idg_restore_launch": (_I, [_P, _P, _P, _P, _P, _P]),
    "idg_ms_scale_radius": (_I, [_D]),
    "idg_ms_scale_taps": (_I, [_D, _I, _P]),
    "idg_convolve_separable": (_I, [_I, _I, _P, _P, _P, _P]),
    "idg_convolve_separable_launch": (_I, [_I, _I, _P, _P, _P, _P, _P]),
    "idg_ms_prepare": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "idg_ms_prepare_launch": (_I, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "idg_ms_clean": (_I, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "idg_ms_clean_launch": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
}


class OptionsStruct(ctypes.Structure):
    """idg_options_t (include/idg_mi355x.h); 0 in a field = unset."""
    _fields_ = [(name, ctypes.c_uint32) for name in (
        "struct_size", "gridder_impl", "degridder_impl", "precision",
        "kernel_form", "fft_fusion", "auto_threshold")]


class PlanParamsStruct(ctypes.Structure):
    """idg_plan_params_t (include/idg_mi355x.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32),
                ("grid_size", ctypes.c_int32),
                ("subgrid_size", ctypes.c_int32),
                ("image_size", ctypes.c_float),
                ("w_step_in_lambda", ctypes.c_float),
                ("nr_w_layers", ctypes.c_int32),
                ("kernel_size", ctypes.c_int32),
                ("max_nr_timesteps_per_subgrid", ctypes.c_int32),
                ("nr_timesteps_per_aterm", ctypes.c_int32)]


class WeightParamsStruct(ctypes.Structure):
    """idg_weight_params_t (include/idg_mi355x.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32),
                ("grid_size", ctypes.c_int32),
                ("image_size", ctypes.c_float),
                ("quantum_log2", ctypes.c_int32),
                ("hermitian", ctypes.c_int32),
                ("scheme", ctypes.c_int32),
                ("robust", ctypes.c_float)]


class CleanParamsStruct(ctypes.Structure):
    """idg_clean_params_t (include/idg_mi355x.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32),
                ("grid_size", ctypes.c_int32),
                ("psf_size", ctypes.c_int32),
                ("max_components", ctypes.c_int32),
                ("nr_iterations", ctypes.c_int32),
                ("gain", ctypes.c_float),
                ("threshold", ctypes.c_float),
                ("cycle_fraction", ctypes.c_float)]


class ClarkParamsStruct(ctypes.Structure):
    """idg_clark_params_t (include/idg_mi355x.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32),
                ("grid_size", ctypes.c_int32),
                ("psf_size", ctypes.c_int32),
                ("max_components", ctypes.c_int32),
                ("nr_rounds", ctypes.c_int32),
                ("iterations_per_round", ctypes.c_int32),
                ("max_candidates", ctypes.c_int32),
                ("gain", ctypes.c_float),
                ("threshold", ctypes.c_float),
                ("cycle_fraction", ctypes.c_float),
                ("select_fraction", ctypes.c_float)]


class MsParamsStruct(ctypes.Structure):
    """idg_ms_params_t (include/idg_mi355x.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32),
                ("grid_size", ctypes.c_int32),
                ("psf_size", ctypes.c_int32),
                ("max_components", ctypes.c_int32),
                ("nr_iterations", ctypes.c_int32),
                ("gain", ctypes.c_float),
                ("threshold", ctypes.c_float),
                ("cycle_fraction", ctypes.c_float),
                ("nr_scales", ctypes.c_int32),
                ("radius", ctypes.c_int32 * 8),
                ("weight", ctypes.c_float * 8),
                ("inv_peak", ctypes.c_float * 8)]


class BeamStruct(ctypes.Structure):
    """idg_beam_t (include/idg_mi355x.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32),
                ("a", ctypes.c_double), ("b", ctypes.c_double),
                ("c", ctypes.c_double), ("major", ctypes.c_double),
                ("minor", ctypes.c_double), ("pa", ctypes.c_double)]


class RestoreParamsStruct(ctypes.Structure):
    """idg_restore_params_t (include/idg_mi355x.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32),
                ("grid_size", ctypes.c_int32),
                ("radius", ctypes.c_int32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with "
            "`make -C ska-sdp-idg-bench_amd` (or __graft_entry__.build()); "
            "the MI355X path has no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()
