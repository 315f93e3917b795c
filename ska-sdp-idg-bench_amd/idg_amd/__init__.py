"""idg_amd -- MI355X-native IDG gridder/degridder (host side).

A Python mirror of the reference's gridder/degridder operator interface over
the C ABI of libidg_mi355x.so (include/idg_mi355x.h).  Importing this package
loads the HIP library and raises if it is missing: there is no CPU fallback.
"""
from .api import (IMAGE_SIZE, METADATA_DTYPE, NR_CORRELATIONS, W_STEP,
                  IdgError, Options, abi_version, auto_selected, adder_launch, as_metadata,
                  bytes_gridder, c_run_degridder, c_run_gridder,
                  degrid_from, degridder_launch, device_name, flops_gridder,
                  generate, grid_onto, gridder_fft_launch, gridder_launch,
                  host_chunk_plan,
                  kernel_name,
                  nr_subgrids_for, plan, plan_launch, precision_options,
                  p_run_degridder, p_run_gridder,
                  release_workspaces,
                  splitter_fft_launch, splitter_launch, subgrid_fft_launch,
                  validate_metadata,
                  grid_fft_launch, grid_to_image, image_to_grid, invert,
                  predict, taper_to_image,
                  psf, weigh, weight_apply, weight_density, weight_scheme,
                  CLEAN_REASONS, COMPONENT_DTYPE, STATE_DTYPE, clean,
                  model_image, stokes_i,
                  CLARK_REASONS, CLARK_STATE_DTYPE, clark,
                  Beam, beam_fit, beam_from_axes, beam_radius, beam_taps,
                  restore,
                  MS_COMPONENT_DTYPE, MS_STATE_DTYPE, clean_multiscale,
                  convolve_separable, ms_clean, ms_prepare, ms_scale_taps,
                  ms_weights)
from ._lib import (LIB_PATH, BeamStruct, ClarkParamsStruct,
                   CleanParamsStruct, MsParamsStruct,
                   OptionsStruct, PlanParamsStruct, RestoreParamsStruct,
                   WeightParamsStruct)
from . import shard

__all__ = [
    "IMAGE_SIZE", "METADATA_DTYPE", "NR_CORRELATIONS", "W_STEP", "IdgError",
    "abi_version", "adder_launch", "as_metadata", "bytes_gridder",
    "c_run_degridder", "c_run_gridder", "degrid_from", "degridder_launch",
    "device_name", "flops_gridder", "generate", "grid_onto",
    "gridder_fft_launch", "gridder_launch", "host_chunk_plan", "kernel_name", "nr_subgrids_for", "p_run_degridder",
    "precision_options", "release_workspaces",
    "p_run_gridder", "splitter_fft_launch", "splitter_launch",
    "subgrid_fft_launch",
    "validate_metadata", "LIB_PATH", "shard", "Options", "OptionsStruct",
    "auto_selected", "plan", "plan_launch", "PlanParamsStruct",
    "grid_fft_launch", "grid_to_image", "image_to_grid", "invert", "predict",
    "taper_to_image",
    "psf", "weigh", "weight_apply", "weight_density", "weight_scheme",
    "WeightParamsStruct",
    "CLEAN_REASONS", "COMPONENT_DTYPE", "STATE_DTYPE", "clean", "model_image",
    "stokes_i", "CleanParamsStruct",
    "CLARK_REASONS", "CLARK_STATE_DTYPE", "clark", "ClarkParamsStruct",
    "Beam", "beam_fit", "beam_from_axes", "beam_radius", "beam_taps",
    "restore", "BeamStruct", "RestoreParamsStruct",
    "MS_COMPONENT_DTYPE", "MS_STATE_DTYPE", "clean_multiscale",
    "convolve_separable", "ms_clean", "ms_prepare", "ms_scale_taps",
    "ms_weights", "MsParamsStruct",
]
