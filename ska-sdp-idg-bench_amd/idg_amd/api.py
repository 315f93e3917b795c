"""Python mirror of the reference's gridder/degridder operator interface.

Same names, argument order and meaning as the reference's kernel-TU contract
(hip::c_run_gridder / hip::c_run_degridder, declared by the harness at
tests/gridder_common.cpp:13-31 and tests/degridder_common.cpp:13-31) and its
perf entries (hip::p_run_gridder / hip::p_run_degridder), over the C ABI of
libidg_mi355x.so.  numpy arrays stand in for the idg::ArrayND objects;
device-resident variants take torch CUDA tensors (PyTorch is only used as the
device allocator / stream provider).

Errors: where the reference's C++ entries abort the process (hipCheck ->
exit, app/HIP/util.cpp:5-15), these raise IdgError carrying the status code
and message.
"""
import collections
import contextlib
import ctypes

import numpy as np

from ._lib import (BeamStruct, ClarkParamsStruct, CleanParamsStruct,
                   MsParamsStruct,
                   OptionsStruct, PlanParamsStruct, RestoreParamsStruct,
                   WeightParamsStruct, lib)

IMAGE_SIZE = 0.01   # app/common/parameters.hpp:4
W_STEP = 0.0        # app/common/parameters.hpp:5
NR_CORRELATIONS = 4

METADATA_DTYPE = np.dtype([("baseline_offset", "<i4"), ("time_offset", "<i4"),
                           ("nr_timesteps", "<i4"), ("aterm_index", "<i4"),
                           ("station1", "<u4"), ("station2", "<u4"),
                           ("x", "<i4"), ("y", "<i4"), ("z", "<i4")])
assert METADATA_DTYPE.itemsize == 36


class IdgError(RuntimeError):
    def __init__(self, code, what):
        msg = lib.idg_last_error().decode(errors="replace")
        super().__init__(f"{what} failed (status {code}): {msg}")
        self.code = code


def _check(code, what):
    if code != 0:
        raise IdgError(code, what)


# ---------------------------------------------------------------------------
# Per-call launch options (idg_options_t)
# ---------------------------------------------------------------------------
IMPLS = {"default": 1, "valu": 2, "sequential": 3, "ordered": 4, "auto": 5}
KERNEL_FORMS = {"combined": 1, "split": 2}
PREC_SET = 8
AUTO_THRESHOLD = 16384


def _enum(value, names, what):
    if value is None:
        return 0
    if isinstance(value, str):
        if value not in names:
            raise ValueError(f"{what} must be one of {sorted(names)}, "
                             f"got {value!r}")
        return names[value]
    return int(value)   # a raw IDG_* value; the library checks it


class Options:
    """Which kernels one call runs, instead of the IDG_* environment
    variables.  None in a field = unset: the variable if it is set, else the
    library's default; an explicit value wins over the variable.

      gridder     "default" | "valu" | "sequential" | "ordered" | "auto"
      degridder   "default" | "sequential"
      precision   0..7, the bits of precision_options()
      kernel_form "combined" | "split"
      fft_fusion  False | True (the FFT in the S = 32 gridder's epilogue)
      auto_threshold  "auto" sends a subgrid to the ordered kernel iff its
                  nr_timesteps x nr_channels exceeds this (library: 16,384)
    """

    def __init__(self, gridder=None, degridder=None, precision=None,
                 kernel_form=None, fft_fusion=None, auto_threshold=None):
        self.gridder = gridder
        self.degridder = degridder
        self.precision = precision
        self.kernel_form = kernel_form
        self.fft_fusion = fft_fusion
        self.auto_threshold = auto_threshold

    def __repr__(self):
        return "Options(" + ", ".join(
            f"{k}={v!r}" for k, v in vars(self).items() if v is not None) + ")"

    def struct(self):
        """The idg_options_t of these options."""
        o = OptionsStruct()
        o.struct_size = ctypes.sizeof(OptionsStruct)
        o.gridder_impl = _enum(self.gridder, IMPLS, "gridder")
        o.degridder_impl = _enum(self.degridder, IMPLS, "degridder")
        if self.precision is not None:
            if not 0 <= int(self.precision) <= 7:
                raise ValueError("precision must be 0..7")
            o.precision = PREC_SET | int(self.precision)
        o.kernel_form = _enum(self.kernel_form, KERNEL_FORMS, "kernel_form")
        if self.fft_fusion is not None:
            o.fft_fusion = 2 if self.fft_fusion else 1
        if self.auto_threshold is not None:
            if not 0 <= int(self.auto_threshold) < 2 ** 32:
                raise ValueError("auto_threshold must fit 32 bits")
            o.auto_threshold = int(self.auto_threshold)
        return o


def _opts_ptr(options):
    """(keep-alive object, pointer) for an Options, a raw OptionsStruct or
    None (NULL: the entries' behaviour without options)."""
    if options is None:
        return None, None
    o = options.struct() if isinstance(options, Options) else options
    if not isinstance(o, OptionsStruct):
        raise TypeError("options must be an idg_amd.Options")
    return o, ctypes.cast(ctypes.pointer(o), ctypes.c_void_p)


def auto_selected(metadata, nr_channels, options=None):
    """The subgrids a gridder="auto" launch with `options` sends to the
    ordered kernel (idg_auto_selected, the host twin of the device
    classification): a uint8 array, 1 = ordered."""
    md = as_metadata(metadata)
    sel = np.zeros(md.size, np.uint8)
    keep, ptr = _opts_ptr(options)
    n = lib.idg_auto_selected(md.size, nr_channels, ptr,
                              _np_ptr(md, METADATA_DTYPE, "metadata"),
                              sel.ctypes.data_as(ctypes.c_void_p))
    if n < 0:
        raise IdgError(n, "auto_selected")
    assert n == int(sel.sum())
    return sel


def _np_ptr(a, dtype, name, writable=False):
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{name} must be a numpy array")
    if a.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {a.dtype}")
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{name} must be C-contiguous")
    if writable and not a.flags["WRITEABLE"]:
        raise ValueError(f"{name} must be writable")
    return a.ctypes.data_as(ctypes.c_void_p)


def as_metadata(md):
    """Accept a METADATA_DTYPE array or an int32 [n, 9] array."""
    md = np.asarray(md)
    if md.dtype == METADATA_DTYPE:
        return np.ascontiguousarray(md)
    md = np.ascontiguousarray(md, dtype=np.int32).reshape(-1, 9)
    return md.view(METADATA_DTYPE).reshape(-1)


def nr_subgrids_for(nr_stations, nr_timeslots):
    return nr_stations * (nr_stations - 1) // 2 * nr_timeslots


# ---------------------------------------------------------------------------
# Synthetic observation (app/common/init.cpp, harness order, srand(0))
# ---------------------------------------------------------------------------
def generate(nr_stations, nr_timeslots, nr_timesteps, nr_channels, grid_size,
             subgrid_size, want=("uvw", "frequencies", "wavenumbers",
                                 "visibilities", "spheroidal", "aterms",
                                 "metadata", "subgrids"), nthreads=8):
    """Return a dict of numpy arrays holding exactly the inputs the reference
    harness builds (tests/gridder_common.cpp:87-101).  Shapes:
      uvw [NS, T, 3] f32; frequencies, wavenumbers [C] f32;
      visibilities [NS, T, C, 4, 2] f32; spheroidal [S, S] f32;
      aterms [TS, ST, S, S, 4, 2] f32; metadata [NS] METADATA_DTYPE;
      subgrids [NS, 4, S, S, 2] f32 (the degridder input ramp)."""
    ns = nr_subgrids_for(nr_stations, nr_timeslots)
    S = subgrid_size
    shapes = {
        "uvw": ((ns, nr_timesteps, 3), np.float32),
        "frequencies": ((nr_channels,), np.float32),
        "wavenumbers": ((nr_channels,), np.float32),
        "visibilities": ((ns, nr_timesteps, nr_channels, 4, 2), np.float32),
        "spheroidal": ((S, S), np.float32),
        "aterms": ((nr_timeslots, nr_stations, S, S, 4, 2), np.float32),
        "metadata": ((ns,), METADATA_DTYPE),
        "subgrids": ((ns, 4, S, S, 2), np.float32),
    }
    out = {k: np.empty(*shapes[k]) for k in want}
    ptr = {k: (out[k].ctypes.data_as(ctypes.c_void_p) if k in out else None)
           for k in shapes}
    got = lib.idg_generate(nr_stations, nr_timeslots, nr_timesteps,
                           nr_channels, grid_size, subgrid_size, ptr["uvw"],
                           ptr["frequencies"], ptr["wavenumbers"],
                           ptr["visibilities"], ptr["spheroidal"],
                           ptr["aterms"], ptr["metadata"], ptr["subgrids"],
                           nthreads)
    if got < 0:
        raise IdgError(got, "idg_generate")
    assert got == ns
    return out


# ---------------------------------------------------------------------------
# Host-buffer entries: hip::c_run_gridder / hip::c_run_degridder
# ---------------------------------------------------------------------------
def _extents(nr_channels, uvw, visibilities, aterms, subgrids, subgrid_size,
             nr_subgrids, nr_stations):
    rows = uvw.size // 3
    if uvw.size % 3:
        raise ValueError("uvw must hold whole (u, v, w) triplets")
    if visibilities.size != rows * nr_channels * 8:
        raise ValueError(
            f"visibilities must hold rows*nr_channels*4 complex values "
            f"({rows}*{nr_channels}*4), got {visibilities.size // 2}")
    per_slot = nr_stations * subgrid_size * subgrid_size * 8
    if aterms.size % per_slot:
        raise ValueError("aterms must be [slots][nr_stations][S][S][4] complex")
    if subgrids.size != nr_subgrids * 4 * subgrid_size * subgrid_size * 2:
        raise ValueError("subgrids must be [nr_subgrids][4][S][S] complex")
    return rows, aterms.size // per_slot


def c_run_gridder(nr_subgrids, grid_size, subgrid_size, image_size,
                  w_step_in_lambda, nr_channels, nr_stations, uvw,
                  wavenumbers, visibilities, spheroidal, aterms, metadata,
                  subgrids, options=None):
    """Grid visibilities onto subgrids (fills `subgrids` in place)."""
    keep, optr = _opts_ptr(options)
    md = as_metadata(metadata)
    rows, slots = _extents(nr_channels, uvw, visibilities, aterms, subgrids,
                           subgrid_size, nr_subgrids, nr_stations)
    _check(lib.idg_c_run_gridder_opts(
        nr_subgrids, grid_size, subgrid_size, image_size, w_step_in_lambda,
        nr_channels, nr_stations, _np_ptr(uvw, np.float32, "uvw"), rows,
        _np_ptr(wavenumbers, np.float32, "wavenumbers"),
        _np_ptr(visibilities, np.float32, "visibilities"),
        _np_ptr(spheroidal, np.float32, "spheroidal"),
        _np_ptr(aterms, np.float32, "aterms"), slots,
        _np_ptr(md, METADATA_DTYPE, "metadata"),
        _np_ptr(subgrids, np.float32, "subgrids", True), optr),
        "c_run_gridder")
    return subgrids


def c_run_degridder(nr_subgrids, grid_size, subgrid_size, image_size,
                    w_step_in_lambda, nr_channels, nr_stations, uvw,
                    wavenumbers, visibilities, spheroidal, aterms, metadata,
                    subgrids, options=None):
    """Degrid subgrids into visibilities (fills `visibilities` in place)."""
    keep, optr = _opts_ptr(options)
    md = as_metadata(metadata)
    rows, slots = _extents(nr_channels, uvw, visibilities, aterms, subgrids,
                           subgrid_size, nr_subgrids, nr_stations)
    _check(lib.idg_c_run_degridder_opts(
        nr_subgrids, grid_size, subgrid_size, image_size, w_step_in_lambda,
        nr_channels, nr_stations, _np_ptr(uvw, np.float32, "uvw"), rows,
        _np_ptr(wavenumbers, np.float32, "wavenumbers"),
        _np_ptr(visibilities, np.float32, "visibilities", True),
        _np_ptr(spheroidal, np.float32, "spheroidal"),
        _np_ptr(aterms, np.float32, "aterms"), slots,
        _np_ptr(md, METADATA_DTYPE, "metadata"),
        _np_ptr(subgrids, np.float32, "subgrids"), optr), "c_run_degridder")
    return visibilities


def validate_metadata(nr_subgrids, subgrid_size, nr_channels, nr_stations,
                      uvw_rows, aterm_slots, metadata):
    md = as_metadata(metadata)
    _check(lib.idg_validate_metadata(
        nr_subgrids, subgrid_size, nr_channels, nr_stations, uvw_rows,
        aterm_slots, _np_ptr(md, METADATA_DTYPE, "metadata")),
        "validate_metadata")


def host_chunk_plan(metadata, bytes_moved):
    """Subgrid bounds of the chunks the host-buffer entries split a batch
    into (idg_host_chunk_plan; util.cpp plan_host_chunks): a list of
    nchunk + 1 subgrid indices."""
    import numpy as np
    md = as_metadata(metadata)
    bounds = np.zeros(18, np.int32)
    n = lib.idg_host_chunk_plan(md.size, _np_ptr(md, METADATA_DTYPE,
                                                  "metadata"),
                                int(bytes_moved), bounds.ctypes.data_as(
                                    ctypes.c_void_p), bounds.size)
    if n < 0:
        _check(n, "host_chunk_plan")
    return [int(b) for b in bounds[:n + 1]]


# ---------------------------------------------------------------------------
# Device-buffer entries (torch CUDA tensors, asynchronous on a stream)
# ---------------------------------------------------------------------------
def _dev_ptr(t, name, dtype=None):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA (HIP) torch tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return ctypes.c_void_p(t.data_ptr())


def _stream_handle(stream):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def _dev_extents(nr_subgrids, subgrid_size, nr_channels, nr_stations, uvw,
                 wavenumbers, visibilities, spheroidal, aterms, metadata,
                 subgrids, validate):
    """Host-side shape checks of a device launch (no device access): every
    tensor must hold exactly the extents the kernel's grid will index.
    With validate=True the metadata is also copied to the host once and
    checked against those extents (idg_validate_metadata: row ranges,
    A-term slots, stations); launches stay asynchronous otherwise, so
    callers that build their own metadata validate it once up front."""
    S, C = subgrid_size, nr_channels
    if uvw.numel() % 3:
        raise ValueError("uvw must hold whole (u, v, w) triplets")
    rows = uvw.numel() // 3
    if visibilities.numel() != rows * C * 8:
        raise ValueError(
            f"visibilities must hold uvw rows x nr_channels x 4 complex "
            f"({rows} x {C} x 4), got {visibilities.numel() // 2}")
    if wavenumbers.numel() < C:
        raise ValueError(f"wavenumbers must hold nr_channels ({C}) values")
    if spheroidal.numel() != S * S:
        raise ValueError(f"spheroidal must be [{S}][{S}]")
    per_slot = nr_stations * S * S * 8
    if aterms.numel() == 0 or aterms.numel() % per_slot:
        raise ValueError("aterms must be [slots][nr_stations][S][S][4] "
                         "complex")
    if metadata.numel() * metadata.element_size() != nr_subgrids * 36:
        raise ValueError(f"metadata must hold nr_subgrids ({nr_subgrids}) "
                         "x 36-byte records")
    if subgrids.numel() != nr_subgrids * 4 * S * S * 2:
        raise ValueError(f"subgrids must be [{nr_subgrids}][4][{S}][{S}] "
                         "complex")
    if validate:
        md = metadata.detach().cpu().contiguous().view(-1).numpy()
        validate_metadata(nr_subgrids, S, C, nr_stations, rows,
                          aterms.numel() // per_slot,
                          np.frombuffer(md.tobytes(), METADATA_DTYPE))


def gridder_launch(nr_subgrids, grid_size, subgrid_size, image_size,
                   w_step_in_lambda, nr_channels, nr_stations, uvw,
                   wavenumbers, visibilities, spheroidal, aterms, metadata,
                   subgrids, stream=None, validate=False, options=None):
    """Enqueue the gridder on device-resident tensors (metadata as int32
    [NS, 9] tensor or uint8 view of METADATA_DTYPE); returns immediately.
    Tensor extents are checked on the host; validate=True also checks the
    metadata (one device-to-host copy)."""
    import torch
    f32 = torch.float32
    _dev_extents(nr_subgrids, subgrid_size, nr_channels, nr_stations, uvw,
                 wavenumbers, visibilities, spheroidal, aterms, metadata,
                 subgrids, validate)
    keep, optr = _opts_ptr(options)
    _check(lib.idg_gridder_launch_opts(
        nr_subgrids, grid_size, subgrid_size, image_size, w_step_in_lambda,
        nr_channels, nr_stations, _dev_ptr(uvw, "uvw", f32),
        _dev_ptr(wavenumbers, "wavenumbers", f32),
        _dev_ptr(visibilities, "visibilities", f32),
        _dev_ptr(spheroidal, "spheroidal", f32),
        _dev_ptr(aterms, "aterms", f32), _dev_ptr(metadata, "metadata"),
        _dev_ptr(subgrids, "subgrids", f32), _stream_handle(stream), optr),
        "gridder_launch")


def gridder_fft_launch(nr_subgrids, grid_size, subgrid_size, image_size,
                       w_step_in_lambda, nr_channels, nr_stations, uvw,
                       wavenumbers, visibilities, spheroidal, aterms, metadata,
                       subgrids, stream=None, validate=False, options=None):
    """gridder_launch followed by subgrid_fft_launch(+1, 1.0): the adder's
    input (uv-domain) subgrids; the FFT runs in the gridder's epilogue for
    S = 32, bit for bit the two launches' result."""
    import torch
    f32 = torch.float32
    _dev_extents(nr_subgrids, subgrid_size, nr_channels, nr_stations, uvw,
                 wavenumbers, visibilities, spheroidal, aterms, metadata,
                 subgrids, validate)
    keep, optr = _opts_ptr(options)
    _check(lib.idg_gridder_fft_launch_opts(
        nr_subgrids, grid_size, subgrid_size, image_size, w_step_in_lambda,
        nr_channels, nr_stations, _dev_ptr(uvw, "uvw", f32),
        _dev_ptr(wavenumbers, "wavenumbers", f32),
        _dev_ptr(visibilities, "visibilities", f32),
        _dev_ptr(spheroidal, "spheroidal", f32),
        _dev_ptr(aterms, "aterms", f32), _dev_ptr(metadata, "metadata"),
        _dev_ptr(subgrids, "subgrids", f32), _stream_handle(stream), optr),
        "gridder_fft_launch")


def degridder_launch(nr_subgrids, grid_size, subgrid_size, image_size,
                     w_step_in_lambda, nr_channels, nr_stations, uvw,
                     wavenumbers, visibilities, spheroidal, aterms, metadata,
                     subgrids, stream=None, validate=False, options=None):
    """Enqueue the degridder on device-resident tensors; returns immediately.
    Extent checks and `validate` as for gridder_launch."""
    import torch
    f32 = torch.float32
    _dev_extents(nr_subgrids, subgrid_size, nr_channels, nr_stations, uvw,
                 wavenumbers, visibilities, spheroidal, aterms, metadata,
                 subgrids, validate)
    keep, optr = _opts_ptr(options)
    _check(lib.idg_degridder_launch_opts(
        nr_subgrids, grid_size, subgrid_size, image_size, w_step_in_lambda,
        nr_channels, nr_stations, _dev_ptr(uvw, "uvw", f32),
        _dev_ptr(wavenumbers, "wavenumbers", f32),
        _dev_ptr(visibilities, "visibilities", f32),
        _dev_ptr(spheroidal, "spheroidal", f32),
        _dev_ptr(aterms, "aterms", f32), _dev_ptr(metadata, "metadata"),
        _dev_ptr(subgrids, "subgrids", f32), _stream_handle(stream), optr),
        "degridder_launch")


# ---------------------------------------------------------------------------
# Pipeline steps either side of the path (not in the
# reference).  gridding:   gridder -> subgrid_fft(+1) -> adder
#              degridding: splitter -> subgrid_fft(-1, 1/S^2) -> degridder
# ---------------------------------------------------------------------------
def _pipe_extents(ns, grid_size, S, nr_w_layers, metadata, subgrids, grid):
    if subgrids.dim() != 5 or tuple(subgrids.shape[1:]) != (4, S, S, 2):
        raise ValueError("subgrids must be [NS][4][S][S][2] float32")
    if metadata.numel() * metadata.element_size() != ns * 36:
        raise ValueError(f"metadata must hold {ns} x 36-byte records")
    if grid.numel() != nr_w_layers * 4 * grid_size * grid_size * 2:
        raise ValueError(f"grid must be [{nr_w_layers}][4][{grid_size}]"
                         f"[{grid_size}][2] float32")


def subgrid_fft_launch(subgrids, sign, scale=1.0, stream=None):
    """In-place 2-D DFT of every [S][S] correlation plane of a float32
    [NS, 4, S, S, 2] tensor: out = scale * sum in * exp(sign 2 pi i ...)."""
    import torch
    ns, _, S = subgrids.shape[0], subgrids.shape[1], subgrids.shape[2]
    _check(lib.idg_subgrid_fft_launch(
        ns, S, int(sign), float(scale),
        _dev_ptr(subgrids, "subgrids", torch.float32), _stream_handle(stream)),
        "subgrid_fft_launch")


def adder_launch(grid_size, metadata, subgrids, grid, nr_w_layers=1,
                 stream=None):
    """grid [W, 4, G, G, 2] float32 += the FFT'd subgrids placed at their
    metadata coordinates.  A deterministic gather: each 16x16 grid tile adds
    the subgrids overlapping it in ascending subgrid order (no atomics on
    the grid)."""
    import torch
    ns, S = subgrids.shape[0], subgrids.shape[2]
    _pipe_extents(ns, grid_size, S, nr_w_layers, metadata, subgrids, grid)
    _check(lib.idg_adder_launch(
        ns, grid_size, S, nr_w_layers, _dev_ptr(metadata, "metadata"),
        _dev_ptr(subgrids, "subgrids", torch.float32),
        _dev_ptr(grid, "grid", torch.float32), _stream_handle(stream)),
        "adder_launch")


def splitter_launch(grid_size, metadata, grid, subgrids, nr_w_layers=1,
                    stream=None):
    """subgrids [NS, 4, S, S, 2] = the uv cells under each subgrid (adjoint
    of adder_launch's placement)."""
    import torch
    ns, S = subgrids.shape[0], subgrids.shape[2]
    _pipe_extents(ns, grid_size, S, nr_w_layers, metadata, subgrids, grid)
    _check(lib.idg_splitter_launch(
        ns, grid_size, S, nr_w_layers, _dev_ptr(metadata, "metadata"),
        _dev_ptr(grid, "grid", torch.float32),
        _dev_ptr(subgrids, "subgrids", torch.float32), _stream_handle(stream)),
        "splitter_launch")


def splitter_fft_launch(grid_size, metadata, grid, subgrids, nr_w_layers=1,
                        stream=None):
    """splitter_launch followed by subgrid_fft_launch(-1, 1/S^2): the
    degridder's input subgrids from the grid (one fused kernel for S = 32 and
    64, bit for bit the two launches' result)."""
    import torch
    ns, S = subgrids.shape[0], subgrids.shape[2]
    _pipe_extents(ns, grid_size, S, nr_w_layers, metadata, subgrids, grid)
    _check(lib.idg_splitter_fft_launch(
        ns, grid_size, S, nr_w_layers, _dev_ptr(metadata, "metadata"),
        _dev_ptr(grid, "grid", torch.float32),
        _dev_ptr(subgrids, "subgrids", torch.float32), _stream_handle(stream)),
        "splitter_fft_launch")


def grid_onto(nr_subgrids, grid_size, subgrid_size, image_size,
              w_step_in_lambda, nr_channels, nr_stations, uvw, wavenumbers,
              visibilities, spheroidal, aterms, metadata, grid,
              nr_w_layers=1, subgrids=None, stream=None, options=None):
    """Visibilities -> uv grid: gridder and subgrid FFT (+1), fused for
    S = 32 (gridder_fft_launch), then the adder into `grid` (accumulates).
    Returns the (uv-domain) subgrid scratch."""
    import torch
    if subgrids is None:
        subgrids = torch.empty((nr_subgrids, 4, subgrid_size, subgrid_size, 2),
                               dtype=torch.float32, device=grid.device)
    gridder_fft_launch(nr_subgrids, grid_size, subgrid_size, image_size,
                       w_step_in_lambda, nr_channels, nr_stations, uvw,
                       wavenumbers, visibilities, spheroidal, aterms,
                       metadata, subgrids, stream, options=options)
    adder_launch(grid_size, metadata, subgrids, grid, nr_w_layers, stream)
    return subgrids


def degrid_from(nr_subgrids, grid_size, subgrid_size, image_size,
                w_step_in_lambda, nr_channels, nr_stations, uvw, wavenumbers,
                visibilities, spheroidal, aterms, metadata, grid,
                nr_w_layers=1, subgrids=None, stream=None, options=None):
    """uv grid -> visibilities: splitter and subgrid FFT (-1, 1/S^2), fused
    for S = 32 / 64 (splitter_fft_launch), then the degridder (overwrites
    the visibility rows of every subgrid)."""
    import torch
    if subgrids is None:
        subgrids = torch.empty((nr_subgrids, 4, subgrid_size, subgrid_size, 2),
                               dtype=torch.float32, device=grid.device)
    splitter_fft_launch(grid_size, metadata, grid, subgrids, nr_w_layers,
                        stream)
    degridder_launch(nr_subgrids, grid_size, subgrid_size, image_size,
                     w_step_in_lambda, nr_channels, nr_stations, uvw,
                     wavenumbers, visibilities, spheroidal, aterms, metadata,
                     subgrids, stream, options=options)
    return subgrids


# ---------------------------------------------------------------------------
# Plan: uvw tracks -> subgrid metadata (idg_plan / idg_plan_launch; not in
# the reference, whose generator draws the coordinates at random)
# ---------------------------------------------------------------------------
def _plan_params(grid_size, subgrid_size, image_size, w_step_in_lambda,
                 kernel_size, max_nr_timesteps_per_subgrid,
                 nr_timesteps_per_aterm, nr_w_layers):
    p = PlanParamsStruct()
    p.struct_size = ctypes.sizeof(PlanParamsStruct)
    p.grid_size = grid_size
    p.subgrid_size = subgrid_size
    p.image_size = image_size
    p.w_step_in_lambda = w_step_in_lambda
    p.nr_w_layers = nr_w_layers
    p.kernel_size = kernel_size
    p.max_nr_timesteps_per_subgrid = max_nr_timesteps_per_subgrid
    p.nr_timesteps_per_aterm = nr_timesteps_per_aterm
    return p


def _plan_shape(uvw_shape, baselines_shape):
    if len(uvw_shape) != 3 or uvw_shape[2] != 3:
        raise ValueError("uvw must be [nr_baselines][nr_timesteps][3]")
    if tuple(baselines_shape) != (uvw_shape[0], 2):
        raise ValueError(f"baselines must be [{uvw_shape[0]}][2] station "
                         "indices")
    return int(uvw_shape[0]), int(uvw_shape[1])


def plan(grid_size, subgrid_size, image_size, w_step_in_lambda, uvw,
         baselines, wavenumbers, kernel_size,
         max_nr_timesteps_per_subgrid=128, nr_timesteps_per_aterm=0,
         nr_w_layers=1, nthreads=8):
    """Cut uvw tracks into subgrids on the host (idg_plan; no device needed).
    uvw: float32 [B, T, 3] in metres, row bl * T + t; baselines: int32 or
    uint32 [B, 2] station indices; wavenumbers: float32 [C], monotone.
    Returns (metadata, dropped): a METADATA_DTYPE array of exactly the
    subgrids needed (baseline-major, time order; time_offset is the first
    uvw row, x / y the corner, z the w layer) and the number of timesteps in
    no subgrid (non-finite, or outside what a subgrid inside the grid with
    kernel_size cells to spare can hold)."""
    B, T = _plan_shape(uvw.shape, baselines.shape)
    if baselines.dtype == np.int32:
        baselines = baselines.view(np.uint32)
    params = _plan_params(grid_size, subgrid_size, image_size,
                          w_step_in_lambda, kernel_size,
                          max_nr_timesteps_per_subgrid,
                          nr_timesteps_per_aterm, nr_w_layers)
    counts = np.zeros(2, np.int32)
    args = (ctypes.cast(ctypes.pointer(params), ctypes.c_void_p), B, T,
            _np_ptr(baselines, np.uint32, "baselines"),
            _np_ptr(uvw, np.float32, "uvw"), wavenumbers.size,
            _np_ptr(wavenumbers, np.float32, "wavenumbers"))
    _check(lib.idg_plan(*args, None, 0, counts.ctypes.data_as(
        ctypes.c_void_p), nthreads), "plan")
    md = np.zeros(int(counts[0]), METADATA_DTYPE)
    if md.size:
        need = int(counts[0])
        _check(lib.idg_plan(*args, _np_ptr(md, METADATA_DTYPE, "metadata",
                                           True), md.size,
                            counts.ctypes.data_as(ctypes.c_void_p), nthreads),
               "plan")
        assert int(counts[0]) == need
    return md, int(counts[1])


def plan_launch(grid_size, subgrid_size, image_size, w_step_in_lambda, uvw,
                baselines, wavenumbers, kernel_size,
                max_nr_timesteps_per_subgrid=128, nr_timesteps_per_aterm=0,
                nr_w_layers=1, metadata=None, capacity=None, stream=None):
    """plan() on device-resident tensors (idg_plan_launch): enqueued on
    `stream`, nothing is read back.  uvw: float32 [B, T, 3]; baselines: int32
    [B, 2]; wavenumbers: float32 [C].  Returns (metadata, counts): an int32
    [capacity, 9] tensor whose first min(counts[0], capacity) records are
    bit for bit plan()'s, and an int32 [2] tensor {subgrids needed, dropped
    timesteps}.  capacity defaults to metadata's records, else to B * T,
    which always suffices; records past counts[0] are left as they were."""
    import torch
    B, T = _plan_shape(tuple(uvw.shape), tuple(baselines.shape))
    if wavenumbers.dim() != 1 or wavenumbers.numel() < 1:
        raise ValueError("wavenumbers must be [nr_channels]")
    if metadata is None:
        if capacity is None:
            capacity = B * T
        metadata = torch.empty((capacity, 9), dtype=torch.int32,
                               device=uvw.device)
    else:
        records = metadata.numel() * metadata.element_size() // 36
        if metadata.numel() * metadata.element_size() % 36:
            raise ValueError("metadata must hold whole 36-byte records")
        if capacity is None:
            capacity = records
        if capacity > records:
            raise ValueError(f"metadata holds {records} records, capacity "
                             f"is {capacity}")
    counts = torch.empty(2, dtype=torch.int32, device=uvw.device)
    params = _plan_params(grid_size, subgrid_size, image_size,
                          w_step_in_lambda, kernel_size,
                          max_nr_timesteps_per_subgrid,
                          nr_timesteps_per_aterm, nr_w_layers)
    _check(lib.idg_plan_launch(
        ctypes.cast(ctypes.pointer(params), ctypes.c_void_p), B, T,
        _dev_ptr(baselines, "baselines", torch.int32),
        _dev_ptr(uvw, "uvw", torch.float32), wavenumbers.numel(),
        _dev_ptr(wavenumbers, "wavenumbers", torch.float32),
        _dev_ptr(metadata, "metadata") if capacity > 0 else None,
        capacity, _dev_ptr(counts, "counts"), _stream_handle(stream)),
        "plan_launch")
    return metadata, counts


# ---------------------------------------------------------------------------
# Grid <-> image (not in the reference): the G x G grid FFT
# with the centre shifts inside its passes, and the w-stacking phasor, the
# sum over the w layers and the taper correction in one launch beside it.
#   invert:  grid_onto -> grid_to_image      predict: image_to_grid -> degrid_from
# ---------------------------------------------------------------------------
MAX_W_LAYERS = 16383    # 4 planes per layer are one launch's grid y (65,535)


def _grid_size_ok(G):
    if not (64 <= G <= 4096 and G & (G - 1) == 0):
        raise ValueError(f"grid_size must be a power of two in [64, 4096], "
                         f"got {G}")


def _image_extents(grid_size, nr_w_layers, correction, grid, image):
    import torch
    G = grid_size
    _grid_size_ok(G)
    if nr_w_layers < 1:
        raise ValueError("nr_w_layers must be >= 1")
    if nr_w_layers > MAX_W_LAYERS:
        raise ValueError(f"nr_w_layers must be <= {MAX_W_LAYERS}")
    if grid.numel() != nr_w_layers * 4 * G * G * 2:
        raise ValueError(f"grid must be [{nr_w_layers}][4][{G}][{G}][2] "
                         "float32")
    if image.numel() != 4 * G * G * 2:
        raise ValueError(f"image must be [4][{G}][{G}][2] float32")
    if correction is None:
        return None
    if correction.numel() != G * G:
        raise ValueError(f"correction must be [{G}][{G}] float32")
    return _dev_ptr(correction, "correction", torch.float32)


def grid_fft_launch(planes, sign, scale=1.0, stream=None):
    """In-place 2-D DFT of every [G][G] plane of a float32 [..., G, G, 2]
    tensor, the definition of subgrid_fft_launch: out[k][l] = scale * sum
    in[y][x] exp(sign 2 pi i (k y + l x) / G); no shift.  G: a power of two
    in [64, 4096]."""
    import torch
    if planes.dim() < 3 or planes.shape[-1] != 2 or \
            planes.shape[-2] != planes.shape[-3]:
        raise ValueError("planes must be [..., G, G, 2] float32")
    G = int(planes.shape[-2])
    _grid_size_ok(G)
    if sign not in (1, -1):
        raise ValueError("sign must be +1 or -1")
    _check(lib.idg_grid_fft_launch(
        G, planes.numel() // (2 * G * G), int(sign), float(scale),
        _dev_ptr(planes, "planes", torch.float32), _stream_handle(stream)),
        "grid_fft_launch")


def grid_to_image(grid_size, image_size, w_step_in_lambda, grid, image=None,
                  nr_w_layers=1, correction=None, stream=None):
    """uv grid [W, 4, G, G, 2] float32 -> image [4, G, G, 2] float32
    (idg_grid_to_image_launch): image = correction * sum_z conj(w phasor of
    layer z) * the centred DFT (sign -1, unscaled) of grid[z].  DESTROYS the
    grid.  correction: float32 [G, G] or None (1).  Returns the image."""
    import torch
    if image is None:
        image = torch.empty((4, grid_size, grid_size, 2), dtype=torch.float32,
                            device=grid.device)
    cptr = _image_extents(grid_size, nr_w_layers, correction, grid, image)
    _check(lib.idg_grid_to_image_launch(
        grid_size, nr_w_layers, image_size, w_step_in_lambda, cptr,
        _dev_ptr(grid, "grid", torch.float32),
        _dev_ptr(image, "image", torch.float32), _stream_handle(stream)),
        "grid_to_image")
    return image


def image_to_grid(grid_size, image_size, w_step_in_lambda, image, grid=None,
                  nr_w_layers=1, correction=None, stream=None):
    """The exact adjoint of grid_to_image (idg_image_to_grid_launch): every
    layer of grid [W, 4, G, G, 2] is overwritten.  Returns the grid."""
    import torch
    if grid is None:
        grid = torch.empty((nr_w_layers, 4, grid_size, grid_size, 2),
                           dtype=torch.float32, device=image.device)
    cptr = _image_extents(grid_size, nr_w_layers, correction, grid, image)
    _check(lib.idg_image_to_grid_launch(
        grid_size, nr_w_layers, image_size, w_step_in_lambda, cptr,
        _dev_ptr(image, "image", torch.float32),
        _dev_ptr(grid, "grid", torch.float32), _stream_handle(stream)),
        "image_to_grid")
    return grid


def taper_to_image(subgrid_size, grid_size, spheroidal):
    """The [S, S] taper as the image sees it (idg_taper_to_image; host, no
    device needed): float64 [G, G], the separable trigonometric interpolant
    of the taper at the image pixels.  correction = 1 / this as float32,
    masked where the caller chooses."""
    sph = np.asarray(spheroidal)
    if sph.shape != (subgrid_size, subgrid_size):
        raise ValueError(f"spheroidal must be [{subgrid_size}]"
                         f"[{subgrid_size}]")
    out = np.empty((max(grid_size, 0), max(grid_size, 0)), np.float64)
    _check(lib.idg_taper_to_image(
        subgrid_size, grid_size, _np_ptr(sph, np.float32, "spheroidal"),
        out.ctypes.data_as(ctypes.c_void_p)), "taper_to_image")
    return out


def _on_stream(stream):
    """torch's current stream set to `stream` (None: left as it is)."""
    import torch
    return (torch.cuda.stream(stream) if stream is not None
            else contextlib.nullcontext())


def invert(nr_subgrids, grid_size, subgrid_size, image_size,
           w_step_in_lambda, nr_channels, nr_stations, uvw, wavenumbers,
           visibilities, spheroidal, aterms, metadata, grid=None,
           nr_w_layers=1, subgrids=None, stream=None, options=None,
           correction=None, image=None, sum_weights=None):
    """Visibilities -> dirty image [4, G, G, 2] float32: grid_onto, then
    grid_to_image.  The exact adjoint of predict; not divided by the number
    of visibilities (one unit visibility with identity A-terms gives modulus
    ~1 everywhere).  grid: None (a zeroed grid is made) or a [W, 4, G, G, 2]
    grid to accumulate onto; it is destroyed.  correction: float32 [G, G]
    (1 / taper_to_image) or None; the 1 / S^2 that undoes the gridding FFT's
    normalisation is folded into it here.  sum_weights: None, or the float64
    device tensor weight_apply / weigh wrote (the sum of the imaging weights):
    the image is divided by it, folded into the same correction on the device
    (nothing is read back), so that a unit point source weighted by weigh()
    images to 1."""
    import torch
    if correction is not None and correction.numel() != grid_size * grid_size:
        raise ValueError(f"correction must be [{grid_size}][{grid_size}] "
                         "float32")
    inv = 1.0 / float(subgrid_size * subgrid_size)
    dev = visibilities.device
    # Everything torch fills or allocates here -- the zeroed grid, the scaled
    # correction, the scratch and the image -- is made with `stream` current,
    # so that the fills are ordered before the kernels enqueued on it.
    with _on_stream(stream):
        if grid is None:
            grid = torch.zeros((nr_w_layers, 4, grid_size, grid_size, 2),
                               dtype=torch.float32, device=dev)
        if correction is None:
            scaled = torch.full((grid_size, grid_size), inv,
                                dtype=torch.float32, device=dev)
        else:
            scaled = (correction.to(torch.float32) * inv).contiguous()
        if sum_weights is not None:
            if sum_weights.numel() != 1 or sum_weights.dtype != torch.float64:
                raise ValueError("sum_weights must be one float64 on the "
                                 "device")
            scaled = (scaled.to(torch.float64) / sum_weights.reshape(())
                      ).to(torch.float32).contiguous()
        grid_onto(nr_subgrids, grid_size, subgrid_size, image_size,
                  w_step_in_lambda, nr_channels, nr_stations, uvw,
                  wavenumbers, visibilities, spheroidal, aterms, metadata,
                  grid, nr_w_layers, subgrids, stream, options)
        return grid_to_image(grid_size, image_size, w_step_in_lambda, grid,
                             image, nr_w_layers, scaled, stream)


def predict(nr_subgrids, grid_size, subgrid_size, image_size,
            w_step_in_lambda, nr_channels, nr_stations, uvw, wavenumbers,
            visibilities, spheroidal, aterms, metadata, image, grid=None,
            nr_w_layers=1, subgrids=None, stream=None, options=None,
            correction=None):
    """Model image [4, G, G, 2] float32 -> visibilities (written for every
    row the metadata covers): image_to_grid, then degrid_from.  One unit
    pixel predicts visibilities of modulus ~1.  grid: scratch [W, 4, G, G, 2]
    or None.  Returns the grid."""
    with _on_stream(stream):    # the scratch is allocated for `stream`
        grid = image_to_grid(grid_size, image_size, w_step_in_lambda, image,
                             grid, nr_w_layers, correction, stream)
        degrid_from(nr_subgrids, grid_size, subgrid_size, image_size,
                    w_step_in_lambda, nr_channels, nr_stations, uvw,
                    wavenumbers, visibilities, spheroidal, aterms, metadata,
                    grid, nr_w_layers, subgrids, stream, options)
    return grid


# ---------------------------------------------------------------------------
# Imaging weights (idg_weight_*; not in the reference): the uv
# sampling density of the samples the gridder will grid, the (a, b) of
# natural / uniform / Briggs weighting, f = w / (a + b D), the weighted
# visibilities and the sum of f.  Each mirror takes numpy arrays (the host
# entry, no device needed) or torch CUDA tensors (the _launch entry,
# asynchronous, nothing read back) and produces the same bytes.
#   weigh: density -> scheme -> apply      psf: apply(None) -> invert
# ---------------------------------------------------------------------------
SCHEMES = {"natural": 0, "uniform": 1, "briggs": 2}
QUANTUM_LOG2 = -20      # weights are counted in units of 2^-20


def _weight_params(grid_size, image_size, quantum_log2, hermitian,
                   scheme="natural", robust=0.0):
    p = WeightParamsStruct()
    p.struct_size = ctypes.sizeof(WeightParamsStruct)
    p.grid_size = grid_size
    p.image_size = image_size
    p.quantum_log2 = quantum_log2
    p.hermitian = 1 if hermitian else 0
    p.scheme = _enum(scheme, SCHEMES, "scheme")
    p.robust = robust
    return p, ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)


def _weight_inputs(uvw, wavenumbers, weights, metadata):
    """(host?, rows, C, nr_subgrids, pointers of uvw / wavenumbers / weights /
    metadata, keep-alive) of a density or apply call, shapes checked."""
    host = isinstance(uvw, np.ndarray)
    if host:
        md = as_metadata(metadata)
        rows, C, ns = uvw.size // 3, wavenumbers.size, md.size
        if uvw.size % 3:
            raise ValueError("uvw must hold whole (u, v, w) triplets")
        if weights.size != rows * C:
            raise ValueError(f"weights must be [{rows}][{C}] float32")
        ptrs = (_np_ptr(uvw, np.float32, "uvw"),
                _np_ptr(wavenumbers, np.float32, "wavenumbers"),
                _np_ptr(weights, np.float32, "weights"),
                _np_ptr(md, METADATA_DTYPE, "metadata"))
        return host, rows, C, ns, ptrs, md
    import torch
    rows, C = uvw.numel() // 3, wavenumbers.numel()
    if uvw.numel() % 3:
        raise ValueError("uvw must hold whole (u, v, w) triplets")
    if weights.numel() != rows * C:
        raise ValueError(f"weights must be [{rows}][{C}] float32")
    nbytes = metadata.numel() * metadata.element_size()
    if nbytes % 36:
        raise ValueError("metadata must hold whole 36-byte records")
    ptrs = (_dev_ptr(uvw, "uvw", torch.float32),
            _dev_ptr(wavenumbers, "wavenumbers", torch.float32),
            _dev_ptr(weights, "weights", torch.float32),
            _dev_ptr(metadata, "metadata") if nbytes else None)
    return host, rows, C, nbytes // 36, ptrs, None


def _density_buffer(host, grid_size, density, device=None):
    G = grid_size
    if host:
        if density is None:
            return np.zeros((G, G), np.uint64)
        if density.size != G * G:
            raise ValueError(f"density must be [{G}][{G}] uint64")
        return density
    import torch
    if density is None:
        return torch.zeros((G, G), dtype=torch.int64, device=device)
    if density.numel() != G * G or density.dtype != torch.int64:
        raise ValueError(f"density must be [{G}][{G}] int64 (the bits of the "
                         "library's uint64)")
    return density


def weight_density(grid_size, subgrid_size, image_size, uvw, wavenumbers,
                   weights, metadata, density=None, quantum_log2=QUANTUM_LOG2,
                   stream=None):
    """density[Y][X] += the sum over the samples the metadata covers of their
    weights in units of 2^quantum_log2, at the nearest uv cell of each sample
    (idg_weight_density / idg_weight_density_launch).  weights: float32
    [rows, C], 0 = flagged.  density: uint64 [G, G] (numpy) / int64 [G, G]
    (torch: the same bits) to accumulate onto, or None for a zeroed one.
    Keep every cell's sum below 2^62.  Exact: the same bits in any order, on
    the host and on the device.  Returns the density."""
    host, rows, C, ns, ptrs, keep = _weight_inputs(uvw, wavenumbers, weights,
                                                   metadata)
    # (a fresh device density is zeroed on `stream`, ahead of the launch)
    with contextlib.nullcontext() if host else _on_stream(stream):
        density = _density_buffer(host, grid_size, density,
                                  None if host else uvw.device)
    p, pp = _weight_params(grid_size, image_size, quantum_log2, True)
    if host:
        _check(lib.idg_weight_density(
            pp, ns, subgrid_size, C, ptrs[3], ptrs[0], rows, ptrs[1], ptrs[2],
            _np_ptr(density, np.uint64, "density", True)), "weight_density")
    else:
        _check(lib.idg_weight_density_launch(
            pp, ns, subgrid_size, C, ptrs[3], ptrs[0], ptrs[1], ptrs[2],
            _dev_ptr(density, "density"), _stream_handle(stream)),
            "weight_density")
    return density


def weight_scheme(grid_size, density, scheme="natural", robust=0.0,
                  quantum_log2=QUANTUM_LOG2, hermitian=True, ab=None,
                  stream=None):
    """(a, b) of f = w / (a + b D) for "natural" (1, 0), "uniform" (0, 1) or
    "briggs" (1, (5 10^-robust)^2 sum D / sum D^2 over all cells) at this
    density (idg_weight_scheme / idg_weight_scheme_launch): float32 [2], a
    numpy array for a numpy density, a device tensor (nothing read back) for a
    device one."""
    p, pp = _weight_params(grid_size, 0.0, quantum_log2, hermitian, scheme,
                           float(robust))
    if isinstance(density, np.ndarray):
        if density.size != grid_size * grid_size:
            raise ValueError("density must be [G][G] uint64")
        if ab is None:
            ab = np.zeros(2, np.float32)
        _check(lib.idg_weight_scheme(
            pp, _np_ptr(density, np.uint64, "density"),
            _np_ptr(ab, np.float32, "ab", True)), "weight_scheme")
        return ab
    import torch
    density = _density_buffer(False, grid_size, density)
    if ab is None:
        with _on_stream(stream):
            ab = torch.zeros(2, dtype=torch.float32, device=density.device)
    _check(lib.idg_weight_scheme_launch(
        pp, _dev_ptr(density, "density"), _dev_ptr(ab, "ab", torch.float32),
        _stream_handle(stream)), "weight_scheme")
    return ab


def weight_apply(grid_size, image_size, uvw, wavenumbers, weights, metadata,
                 density, ab, visibilities=None, imaging_weights=None,
                 out=None, sum_weights=None, quantum_log2=QUANTUM_LOG2,
                 hermitian=True, stream=None):
    """For every sample the metadata covers: imaging_weights = f =
    w / (a + b D), out = f * visibilities ((f, 0, 0, f) with visibilities
    None, the PSF's input; literal zeros for a flagged sample), sum_weights =
    sum f in float64 (idg_weight_apply / idg_weight_apply_launch).  out may
    be visibilities.  Rows no subgrid covers are left as they were; buffers
    made here start as zeros.  Returns (imaging_weights [rows, C], out
    [rows, C, 4, 2], sum_weights [1] float64)."""
    host, rows, C, ns, ptrs, keep = _weight_inputs(uvw, wavenumbers, weights,
                                                   metadata)
    p, pp = _weight_params(grid_size, image_size, quantum_log2, hermitian)
    if visibilities is not None and (
            (visibilities.size if host else visibilities.numel())
            != rows * C * 8):
        raise ValueError(f"visibilities must be [{rows}][{C}][4] complex")
    if host:
        if imaging_weights is None:
            imaging_weights = np.zeros((rows, C), np.float32)
        if out is None:
            out = np.zeros((rows, C, 4, 2), np.float32)
        if sum_weights is None:
            sum_weights = np.zeros(1, np.float64)
        if imaging_weights.size != rows * C or out.size != rows * C * 8:
            raise ValueError("imaging_weights must be [rows][C], out "
                             "[rows][C][4] complex")
        _check(lib.idg_weight_apply(
            pp, ns, C, ptrs[3], ptrs[0], rows, ptrs[1], ptrs[2],
            _np_ptr(density, np.uint64, "density"),
            _np_ptr(ab, np.float32, "ab"),
            None if visibilities is None else _np_ptr(
                visibilities, np.float32, "visibilities"),
            _np_ptr(imaging_weights, np.float32, "imaging_weights", True),
            _np_ptr(out, np.float32, "out", True),
            _np_ptr(sum_weights, np.float64, "sum_weights", True)),
            "weight_apply")
        return imaging_weights, out, sum_weights
    import torch
    dev = uvw.device
    density = _density_buffer(False, grid_size, density)
    with _on_stream(stream):
        if imaging_weights is None:
            imaging_weights = torch.zeros((rows, C), dtype=torch.float32,
                                          device=dev)
        if out is None:
            out = torch.zeros((rows, C, 4, 2), dtype=torch.float32,
                              device=dev)
        if sum_weights is None:
            sum_weights = torch.zeros(1, dtype=torch.float64, device=dev)
    if imaging_weights.numel() != rows * C or out.numel() != rows * C * 8:
        raise ValueError("imaging_weights must be [rows][C], out "
                         "[rows][C][4] complex")
    _check(lib.idg_weight_apply_launch(
        pp, ns, C, ptrs[3], ptrs[0], ptrs[1], ptrs[2],
        _dev_ptr(density, "density"), _dev_ptr(ab, "ab", torch.float32),
        None if visibilities is None else _dev_ptr(
            visibilities, "visibilities", torch.float32),
        _dev_ptr(imaging_weights, "imaging_weights", torch.float32),
        _dev_ptr(out, "out", torch.float32),
        _dev_ptr(sum_weights, "sum_weights", torch.float64),
        _stream_handle(stream)), "weight_apply")
    return imaging_weights, out, sum_weights


def weigh(grid_size, subgrid_size, image_size, uvw, wavenumbers, weights,
          metadata, visibilities=None, scheme="natural", robust=0.0,
          density=None, out=None, quantum_log2=QUANTUM_LOG2, hermitian=True,
          stream=None):
    """weight_density -> weight_scheme -> weight_apply in one go, on the
    device with nothing read back between the steps (or on the host, for
    numpy inputs).  density: None (this batch's own) or one to accumulate
    onto first.  Returns (imaging_weights, weighted visibilities,
    sum_weights, density, ab)."""
    with (contextlib.nullcontext() if isinstance(uvw, np.ndarray)
          else _on_stream(stream)):
        density = weight_density(grid_size, subgrid_size, image_size, uvw,
                                 wavenumbers, weights, metadata, density,
                                 quantum_log2, stream)
        ab = weight_scheme(grid_size, density, scheme, robust, quantum_log2,
                           hermitian, None, stream)
        iw, out, total = weight_apply(
            grid_size, image_size, uvw, wavenumbers, weights, metadata,
            density, ab, visibilities, None, out, None, quantum_log2,
            hermitian, stream)
    return iw, out, total, density, ab


def psf(grid_size, subgrid_size, image_size, w_step_in_lambda, nr_stations,
        uvw, wavenumbers, weights, spheroidal, metadata, scheme="natural",
        robust=0.0, density=None, nr_w_layers=1, aterm_slots=1,
        correction=None, quantum_log2=QUANTUM_LOG2, hermitian=True,
        stream=None, options=None):
    """The point spread function [4, G, G, 2] float32 of these samples under
    a weighting scheme, on the device: weigh() with no visibilities (each
    covered sample becomes (f, 0, 0, f)), then invert() with identity
    A-terms and sum_weights, so the centre pixel of xx and yy is 1 (as far as
    `correction` undoes the taper there).  aterm_slots: the A-term slots the
    metadata refers to.  density: as for weigh()."""
    import torch
    S, C = subgrid_size, wavenumbers.numel()
    ns = metadata.numel() * metadata.element_size() // 36
    with _on_stream(stream):
        iw, vis, total, density, ab = weigh(
            grid_size, S, image_size, uvw, wavenumbers, weights, metadata,
            None, scheme, robust, density, None, quantum_log2, hermitian,
            stream)
        aterms = torch.zeros((aterm_slots, nr_stations, S, S, 4, 2),
                             dtype=torch.float32, device=uvw.device)
        aterms[..., 0, 0] = 1.0
        aterms[..., 3, 0] = 1.0
        return invert(ns, grid_size, S, image_size, w_step_in_lambda, C,
                      nr_stations, uvw, wavenumbers, vis, spheroidal, aterms,
                      metadata, nr_w_layers=nr_w_layers, stream=stream,
                      options=options, correction=correction,
                      sum_weights=total)


# ---------------------------------------------------------------------------
# Hogbom CLEAN minor cycle (idg_clean / idg_clean_launch; not
# in the reference): dirty image -> model on one real plane.  numpy arrays
# take the host entry, torch CUDA tensors the _launch entry (asynchronous);
# the same bytes either way.
#   stokes_i(invert(...)), stokes_i(psf(...)) -> clean -> model_image ->
#   predict
# ---------------------------------------------------------------------------
COMPONENT_DTYPE = np.dtype([("y", "<i4"), ("x", "<i4"), ("value", "<f4")])
STATE_DTYPE = np.dtype([("n_components", "<i4"), ("reason", "<i4"),
                        ("started", "<i4"), ("peak_index", "<i4"),
                        ("level", "<f4"), ("peak", "<f4")])
assert COMPONENT_DTYPE.itemsize == 12 and STATE_DTYPE.itemsize == 24
CLEAN_REASONS = {0: "running", 1: "below_level", 2: "no_peak",
                 3: "components_full"}


def stokes_i(image):
    """[4, G, G, 2] (xx, xy, yx, yy as re / im pairs) -> [G, G] float32,
    0.5 * (Re xx + Re yy): the plane clean() works on, of invert()'s image and
    of psf()'s alike.  numpy or torch."""
    if tuple(image.shape[:1]) != (4,) or tuple(image.shape[3:]) != (2,):
        raise ValueError("image must be [4, G, G, 2]")
    return 0.5 * (image[0, :, :, 0] + image[3, :, :, 0])


def model_image(model):
    """[G, G] -> [4, G, G, 2] float32 with xx = yy = model and the rest 0:
    predict()'s input for an unpolarised model.  numpy or torch."""
    if model.ndim != 2:
        raise ValueError("model must be [G, G]")
    if isinstance(model, np.ndarray):
        out = np.zeros((4,) + model.shape + (2,), np.float32)
    else:
        import torch
        out = torch.zeros((4,) + tuple(model.shape) + (2,),
                          dtype=torch.float32, device=model.device)
    out[0, :, :, 0] = model
    out[3, :, :, 0] = model
    return out


def _clean_params(G, Gp, max_components, nr_iterations, gain, threshold,
                  cycle_fraction):
    p = CleanParamsStruct()
    p.struct_size = ctypes.sizeof(CleanParamsStruct)
    p.grid_size, p.psf_size = G, Gp
    p.max_components, p.nr_iterations = max_components, nr_iterations
    p.gain, p.threshold, p.cycle_fraction = gain, threshold, cycle_fraction
    return p, ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)


def _square(a, name):
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"{name} must be a square plane, got "
                         f"{tuple(a.shape)}")
    return a.shape[0]


def _minor_cycle(what, entries, params, lead, G, dtypes, model, mask,
                 max_components, nr_iterations, components, state,
                 check_every, stream):
    """What clean() and ms_clean() share.  entries: the (host, _launch) pair
    of the C ABI, called as entry(params(n)[1], *lead, mask, model,
    components, state[, stream]) for n iterations; lead: the (buffer, name,
    written) triples the entry takes first, all float32, numpy for the host
    entry; dtypes: the numpy (component, state) records.  Makes the model,
    components and state that are None, refuses wrong shapes and dtypes,
    passes a bool mask as uint8 and, on the device, enqueues check_every
    iterations at a time.  Returns (model, components, state)."""
    host = isinstance(lead[0][0], np.ndarray)
    records = max(max_components, 1)     # (never a null pointer)
    if host:
        if model is None:
            model = np.zeros((G, G), np.float32)
        if components is None:
            components = np.zeros(records, dtypes[0])
        if state is None:
            state = np.zeros(1, dtypes[1])
        if (model.shape != (G, G) or components.size < max_components
                or state.size != 1
                or (mask is not None and mask.shape != (G, G))):
            raise ValueError("model and mask must be [G][G], components "
                             "[max_components], state [1]")
        if mask is not None and mask.dtype == np.bool_:
            mask = mask.view(np.uint8)
        p, pp = params(nr_iterations)
        _check(entries[0](
            pp, *(_np_ptr(a, np.float32, name, written)
                  for a, name, written in lead),
            None if mask is None else _np_ptr(mask, np.uint8, "mask"),
            _np_ptr(model, np.float32, "model", True),
            _np_ptr(components, dtypes[0], "components", True),
            _np_ptr(state, dtypes[1], "state", True)), what)
        return model, components, state
    import torch
    dev = lead[0][0].device
    # a record as int32s
    width, fields = dtypes[0].itemsize // 4, dtypes[1].itemsize // 4
    with _on_stream(stream):
        if model is None:
            model = torch.zeros((G, G), dtype=torch.float32, device=dev)
        if components is None:
            components = torch.zeros((records, width), dtype=torch.int32,
                                     device=dev)
        if state is None:
            state = torch.zeros(fields, dtype=torch.int32, device=dev)
    if (tuple(model.shape) != (G, G) or components.numel() < width *
            max_components or state.numel() != fields
            or (mask is not None and tuple(mask.shape) != (G, G))):
        raise ValueError("model and mask must be [G][G], components "
                         f"[max_components][{width}] int32, state [{fields}] "
                         "int32")
    if mask is not None and mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError("mask must be uint8 or bool")
    ptrs = [_dev_ptr(a, name, torch.float32) for a, name, _ in lead] + [
        None if mask is None else _dev_ptr(mask, "mask"),
        _dev_ptr(model, "model", torch.float32),
        _dev_ptr(components, "components", torch.int32),
        _dev_ptr(state, "state", torch.int32)]
    if check_every is not None and check_every < 1:
        raise ValueError("check_every must be at least 1")
    chunk = nr_iterations if check_every is None else check_every
    left = nr_iterations
    while True:
        n = min(chunk, left)
        p, pp = params(n)
        _check(entries[1](pp, *ptrs, _stream_handle(stream)), what)
        left -= n
        if left == 0:
            break
        with _on_stream(stream):    # the copy waits for `stream`, and only it
            if int(state[1:2].cpu()) != 0:
                break
    return model, components, state


def clean(residual, psf,model=None, mask=None, gain=0.1, threshold=0.0,
          cycle_fraction=0.0, max_components=1000, nr_iterations=None,
          components=None, state=None, check_every=None, stream=None):
    """Hogbom minor cycle (idg_clean / idg_clean_launch): up to nr_iterations
    (None: max_components) times, take gain * the peak of `residual` as a
    component, add it to `model` and subtract it times `psf` around the peak,
    until the peak is no longer above max(threshold, cycle_fraction * the
    first peak), no searchable pixel is left or `components` is full.
    residual: float32 [G, G], updated in place.  psf: float32 [Gp, Gp], Gp <=
    G, centre (Gp // 2, Gp // 2) of value 1 (psf() makes it so).  mask: uint8
    or bool [G, G] or None: where 0, no peak is searched (the subtraction
    goes everywhere).  model: float32 [G, G] to accumulate onto, or None for a
    zeroed one.  components / state: None for fresh ones, or those of an
    earlier call to continue it: k calls of n iterations give the bytes of one
    call of k * n.  numpy: COMPONENT_DTYPE [max_components] and STATE_DTYPE
    [1]; torch: the same bytes as int32 [max_components, 3] and int32 [6]
    (view the float fields with .view(torch.float32)).  check_every = n
    (device only): n iterations are enqueued at a time and the 4 bytes of
    state.reason read back between the chunks, to stop enqueueing once it is
    set; None reads nothing back.  Returns (residual, model, components,
    state)."""
    G, Gp = _square(residual, "residual"), _square(psf, "psf")
    if nr_iterations is None:
        nr_iterations = max_components

    def params(n):
        return _clean_params(G, Gp, max_components, n, gain, threshold,
                             cycle_fraction)
    model, components, state = _minor_cycle(
        "clean", (lib.idg_clean, lib.idg_clean_launch), params,
        [(residual, "residual", True), (psf, "psf", False)], G,
        (COMPONENT_DTYPE, STATE_DTYPE), model, mask, max_components,
        nr_iterations, components, state, check_every, stream)
    return residual, model, components, state


# ---------------------------------------------------------------------------
# Clark CLEAN (idg_clark / idg_clark_launch; not in the
# reference): clean()'s minor cycle on a list of the brightest pixels, many
# components per launch.  numpy arrays take the host entry, torch CUDA tensors
# the _launch entry (asynchronous); the same bytes either way.
#   ... -> clark(residual, psf) -> model_image -> predict
# ---------------------------------------------------------------------------
CLARK_STATE_DTYPE = np.dtype(STATE_DTYPE.descr + [
    ("n_candidates", "<i4"), ("round_limit", "<f4"), ("rounds", "<i4")])
assert CLARK_STATE_DTYPE.itemsize == 36
CLARK_REASONS = {**CLEAN_REASONS, 4: "no_candidate"}


def _clark_params(G, Gp, max_components, nr_rounds, iterations_per_round,
                  max_candidates, gain, threshold, cycle_fraction,
                  select_fraction):
    p = ClarkParamsStruct()
    p.struct_size = ctypes.sizeof(ClarkParamsStruct)
    p.grid_size, p.psf_size = G, Gp
    p.max_components, p.nr_rounds = max_components, nr_rounds
    p.iterations_per_round = iterations_per_round
    p.max_candidates = max_candidates
    p.gain, p.threshold, p.cycle_fraction = gain, threshold, cycle_fraction
    p.select_fraction = select_fraction
    return p, ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)


def clark(residual, psf, model=None, mask=None, gain=0.1, threshold=0.0,
          cycle_fraction=0.0, select_fraction=0.3, max_candidates=4096,
          iterations_per_round=1000, max_components=1000, nr_rounds=None,
          components=None, state=None, check_every=None, stream=None):
    """Clark CLEAN (idg_clark / idg_clark_launch): nr_rounds rounds, each of
    which lists the pixels of `residual` above max(level, select_fraction *
    the peak) -- at most max_candidates of them, the limit raised to a
    histogram bin's edge where more would qualify --, runs clean()'s minor
    cycle on that list for up to iterations_per_round components and then
    subtracts those components from the whole residual.  On the device a
    round is five launches however many components it takes.  It stops as
    clean() does, or with reason 4 when a round's list is empty.
    residual, psf, mask, model, components, gain, threshold, cycle_fraction
    and max_components: as for clean().  state: None for a fresh one, or that
    of an earlier call to continue it: k calls of n rounds give the bytes of
    one call of k * n.  numpy: CLARK_STATE_DTYPE [1]; torch: the same bytes as
    int32 [9].  nr_rounds = None: rounds until state.reason is set, at most
    max_components + 1 (iterations_per_round must then be at least 1, so that
    a round takes a component or sets a reason); on the device that takes
    check_every, which then defaults to 1.  check_every = n (device only): n
    rounds are enqueued at a time and the 4 bytes of state.reason read back
    between the chunks; None reads nothing back.  Returns (residual, model,
    components, state)."""
    G, Gp = _square(residual, "residual"), _square(psf, "psf")
    if nr_rounds is None:
        if iterations_per_round < 1:
            raise ValueError("nr_rounds=None needs iterations_per_round >= 1")
        # a round takes a component or sets a reason: these rounds suffice,
        # and the loop ends on a state the launch form runs no round from
        nr_rounds = max_components + 1
        if check_every is None and not isinstance(residual, np.ndarray):
            check_every = 1

    def params(n):
        return _clark_params(G, Gp, max_components, n, iterations_per_round,
                             max_candidates, gain, threshold, cycle_fraction,
                             select_fraction)
    model, components, state = _minor_cycle(
        "clark", (lib.idg_clark, lib.idg_clark_launch), params,
        [(residual, "residual", True), (psf, "psf", False)], G,
        (COMPONENT_DTYPE, CLARK_STATE_DTYPE), model, mask, max_components,
        nr_rounds, components, state, check_every, stream)
    return residual, model, components, state


# ---------------------------------------------------------------------------
# Multi-scale CLEAN (idg_ms_* / idg_convolve_separable; not in
# the reference).  numpy planes take the host entries, torch CUDA tensors the
# _launch entries (asynchronous); the same bytes either way.
#   ... -> clean_multiscale(residual, psf) -> restore(model, residual, ...)
# ---------------------------------------------------------------------------
MS_COMPONENT_DTYPE = np.dtype([("y", "<i4"), ("x", "<i4"), ("scale", "<i4"),
                               ("value", "<f4")])
MS_STATE_DTYPE = np.dtype(STATE_DTYPE.descr + [("peak_scale", "<i4")])
assert MS_COMPONENT_DTYPE.itemsize == 16 and MS_STATE_DTYPE.itemsize == 28
MS_MAX_SCALES = 8


def ms_scale_taps(scales):
    """The 1-D taps of every scale (idg_ms_scale_radius / idg_ms_scale_taps;
    host only, in doubles): a list of float32 arrays [2 r + 1], r = ceil(3
    sigma), sigma = scale * 3 / 16; scale 0 gives [1.0].  The 2-D kernel of a
    scale is the outer product of its taps with themselves."""
    out = []
    for a in scales:
        r = lib.idg_ms_scale_radius(float(a))
        if r < 0:
            raise IdgError(r, "ms_scale_taps")
        taps = np.empty(2 * r + 1, np.float32)
        _check(lib.idg_ms_scale_taps(float(a), r,
                                     _np_ptr(taps, np.float32, "taps", True)),
               "ms_scale_taps")
        out.append(taps)
    return out


def _ms_taps(taps):
    """A list of per-scale tap arrays -> (radii, the concatenated table)."""
    taps = [np.ascontiguousarray(t, np.float32).reshape(-1) for t in taps]
    if not 1 <= len(taps) <= MS_MAX_SCALES:
        raise ValueError("1 to 8 scales")
    if any(t.size % 2 != 1 for t in taps):
        raise ValueError("a scale's taps must be [2 r + 1]")
    return [t.size // 2 for t in taps], np.concatenate(taps)


def _ms_params(G, Gp, radii, max_components=0, nr_iterations=0, gain=0.0,
               threshold=0.0, cycle_fraction=0.0, weight=None, inv_peak=None):
    p = MsParamsStruct()
    p.struct_size = ctypes.sizeof(MsParamsStruct)
    p.grid_size, p.psf_size, p.nr_scales = G, Gp, len(radii)
    p.max_components, p.nr_iterations = max_components, nr_iterations
    p.gain, p.threshold, p.cycle_fraction = gain, threshold, cycle_fraction
    for s, r in enumerate(radii):
        p.radius[s] = r
        p.weight[s] = 1.0 if weight is None else weight[s]
        p.inv_peak[s] = 1.0 if inv_peak is None else inv_peak[s]
    return p, ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)


def _to_device(a, like, stream):
    import torch
    with _on_stream(stream):
        return torch.from_numpy(a).to(like.device, non_blocking=True)


def convolve_separable(image, taps, out=None, tmp=None, stream=None):
    """Dense separable convolution (idg_convolve_separable / _launch): `image`
    float32 [G, G], zero beyond its edge, with the outer product of `taps`
    (float32 [2 r + 1], r <= 48; numpy, uploaded on `stream` for CUDA planes,
    or a CUDA tensor): a row pass into `tmp`, a column pass into `out`, every
    pixel's taps taken in ascending order with one fmaf each.  out: None for a
    new plane; it may be `image`.  tmp: a [G, G] scratch plane distinct from
    both, None for a new one.  Returns out."""
    host = isinstance(image, np.ndarray)
    G = _square(image, "image")
    if taps.ndim != 1 or taps.shape[0] % 2 != 1:
        raise ValueError("taps must be [2 r + 1]")
    r = taps.shape[0] // 2
    if host:
        out = np.empty((G, G), np.float32) if out is None else out
        tmp = np.empty((G, G), np.float32) if tmp is None else tmp
        if out.shape != image.shape or tmp.shape != image.shape:
            raise ValueError("out and tmp must be [G][G]")
        _check(lib.idg_convolve_separable(
            G, r, _np_ptr(image, np.float32, "image"),
            _np_ptr(taps, np.float32, "taps"),
            _np_ptr(tmp, np.float32, "tmp", True),
            _np_ptr(out, np.float32, "out", True)), "convolve_separable")
        return out
    import torch
    if isinstance(taps, np.ndarray):
        taps = _to_device(np.ascontiguousarray(taps, np.float32), image,
                          stream)
    with _on_stream(stream):
        if out is None:
            out = torch.empty_like(image)
        if tmp is None:
            tmp = torch.empty_like(image)
    if out.shape != image.shape or tmp.shape != image.shape:
        raise ValueError("out and tmp must be [G][G]")
    _check(lib.idg_convolve_separable_launch(
        G, r, _dev_ptr(image, "image", torch.float32),
        _dev_ptr(taps, "taps", torch.float32),
        _dev_ptr(tmp, "tmp", torch.float32),
        _dev_ptr(out, "out", torch.float32), _stream_handle(stream)),
        "convolve_separable")
    return out


def ms_prepare(residual, psf, taps, planes=None, cross_psf=None, tmp=None,
               stream=None):
    """The scale planes and the cross-PSFs (idg_ms_prepare / _launch), once
    per major cycle.  residual float32 [G, G], psf float32 [Gp, Gp], taps: the
    list ms_scale_taps makes (the first scale must be 0).  planes [Ns, G, G]:
    planes[0] a copy of the residual, planes[s] the residual convolved with
    scale s.  cross_psf [Ns (Ns + 1) / 2, Gp, Gp]: the PSF convolved with
    scales s and q, s <= q, row-major over the pairs, truncated to the PSF's
    window.  None: new buffers; tmp: a [G, G] scratch plane.  Returns (planes,
    cross_psf)."""
    host = isinstance(residual, np.ndarray)
    G, Gp = _square(residual, "residual"), _square(psf, "psf")
    radii, table = _ms_taps(taps)
    Ns = len(radii)
    pairs = Ns * (Ns + 1) // 2
    p, pp = _ms_params(G, Gp, radii)
    if host:
        planes = np.empty((Ns, G, G), np.float32) if planes is None else planes
        if cross_psf is None:
            cross_psf = np.empty((pairs, Gp, Gp), np.float32)
        tmp = np.empty((G, G), np.float32) if tmp is None else tmp
        if (planes.shape != (Ns, G, G) or cross_psf.shape != (pairs, Gp, Gp)
                or tmp.shape != (G, G)):
            raise ValueError("planes must be [Ns][G][G], cross_psf "
                             "[Ns (Ns + 1) / 2][Gp][Gp], tmp [G][G]")
        _check(lib.idg_ms_prepare(
            pp, _np_ptr(residual, np.float32, "residual"),
            _np_ptr(psf, np.float32, "psf"),
            _np_ptr(table, np.float32, "taps"),
            _np_ptr(planes, np.float32, "planes", True),
            _np_ptr(cross_psf, np.float32, "cross_psf", True),
            _np_ptr(tmp, np.float32, "tmp", True)), "ms_prepare")
        return planes, cross_psf
    import torch
    table = _to_device(table, residual, stream)
    with _on_stream(stream):
        kw = dict(dtype=torch.float32, device=residual.device)
        if planes is None:
            planes = torch.empty((Ns, G, G), **kw)
        if cross_psf is None:
            cross_psf = torch.empty((pairs, Gp, Gp), **kw)
        if tmp is None:
            tmp = torch.empty((G, G), **kw)
    if (tuple(planes.shape) != (Ns, G, G)
            or tuple(cross_psf.shape) != (pairs, Gp, Gp)
            or tuple(tmp.shape) != (G, G)):
        raise ValueError("planes must be [Ns][G][G], cross_psf "
                         "[Ns (Ns + 1) / 2][Gp][Gp], tmp [G][G]")
    _check(lib.idg_ms_prepare_launch(
        pp, _dev_ptr(residual, "residual", torch.float32),
        _dev_ptr(psf, "psf", torch.float32),
        _dev_ptr(table, "taps", torch.float32),
        _dev_ptr(planes, "planes", torch.float32),
        _dev_ptr(cross_psf, "cross_psf", torch.float32),
        _dev_ptr(tmp, "tmp", torch.float32), _stream_handle(stream)),
        "ms_prepare")
    return planes, cross_psf


def ms_clean(planes, cross_psf, taps, weight, inv_peak, model=None, mask=None,
             gain=0.1, threshold=0.0, cycle_fraction=0.0, max_components=1000,
             nr_iterations=None, components=None, state=None,
             check_every=None, stream=None):
    """The multi-scale minor cycle on prepared planes (idg_ms_clean /
    _launch), the entry clean_multiscale() is built on.  planes [Ns, G, G] and
    cross_psf [Ns (Ns + 1) / 2, Gp, Gp], both updated / read as ms_prepare
    leaves them; taps: ms_scale_taps' list; weight, inv_peak: Ns floats each,
    what a plane's values are multiplied by for the search and a component's
    value for its flux.  model, mask, components, state, nr_iterations,
    check_every as for clean(); numpy: MS_COMPONENT_DTYPE and MS_STATE_DTYPE
    records; torch: int32 [max_components, 4] and int32 [7].  Returns (planes,
    model, components, state)."""
    host = isinstance(planes, np.ndarray)
    if planes.ndim != 3 or cross_psf.ndim != 3:
        raise ValueError("planes must be [Ns][G][G], cross_psf "
                         "[Ns (Ns + 1) / 2][Gp][Gp]")
    radii, table = _ms_taps(taps)
    Ns = len(radii)
    G, Gp = _square(planes[0], "planes"), _square(cross_psf[0], "cross_psf")
    if (planes.shape[0] != Ns or cross_psf.shape[0] != Ns * (Ns + 1) // 2
            or len(weight) != Ns or len(inv_peak) != Ns):
        raise ValueError("planes, cross_psf, weight and inv_peak must match "
                         "the number of scales")
    if nr_iterations is None:
        nr_iterations = max_components

    def params(n):
        return _ms_params(G, Gp, radii, max_components, n, gain, threshold,
                          cycle_fraction, weight, inv_peak)
    if not host:
        table = _to_device(table, planes, stream)
    model, components, state = _minor_cycle(
        "ms_clean", (lib.idg_ms_clean, lib.idg_ms_clean_launch), params,
        [(planes, "planes", True), (cross_psf, "cross_psf", False),
         (table, "taps", False)], G, (MS_COMPONENT_DTYPE, MS_STATE_DTYPE),
        model, mask, max_components, nr_iterations, components, state,
        check_every, stream)
    return planes, model, components, state


def ms_weights(cross_psf, scales, scale_bias=0.6):
    """clean_multiscale's default (weight, inv_peak), in doubles and rounded
    once to float32: inv_peak[s] = 1 / cross(s, s)[centre] and weight[s] =
    (1 - scale_bias * a_s / a_max) * inv_peak[s] (the bias factor is 1 when
    a_max = 0).  For a CUDA cross_psf the Ns centre values are copied to the
    host, which synchronises with the current stream."""
    Ns = len(scales)
    Gp = cross_psf.shape[-1]
    at = [s * Ns - s * (s - 1) // 2 for s in range(Ns)]
    centre = cross_psf[at, Gp // 2, Gp // 2]
    if not isinstance(centre, np.ndarray):
        centre = centre.cpu().numpy()
    a_max = float(max(scales))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / centre.astype(np.float64)
        bias = np.array([1.0 if a_max == 0 else
                         1.0 - scale_bias * float(a) / a_max for a in scales])
        return ((bias * inv).astype(np.float32), inv.astype(np.float32))


def clean_multiscale(residual, psf, scales=(0, 4, 8, 16), scale_bias=0.6,
                     model=None, mask=None, gain=0.1, threshold=0.0,
                     cycle_fraction=0.0, max_components=1000,
                     nr_iterations=None, components=None, state=None,
                     planes=None, cross_psf=None, check_every=None,
                     stream=None):
    """Multi-scale CLEAN minor cycle (Cornwell 2008): clean() with components
    that are Gaussian blobs of the widths `scales` (pixels, ascending, the
    first 0: the point component; a scale a has sigma = 3 a / 16).  residual,
    psf, model, mask, gain, threshold, cycle_fraction, max_components,
    nr_iterations, components, state, check_every: as for clean(), with
    MS_COMPONENT_DTYPE / MS_STATE_DTYPE records (torch: int32 [., 4] and int32
    [7]) and the threshold applying to the scale-weighted peak, which for
    scale 0 is the residual's own value.  The model receives every
    component's blob, so model_image() and restore() take it unchanged.

    Without `planes` the scale planes and cross-PSFs are made first
    (ms_prepare).  With `planes` and `cross_psf` from an earlier call the
    cycle continues from them, which is how a chunked run works; `residual`
    is then only written.  At the end `residual` receives planes[0], in
    place.  The search weights are ms_weights(cross_psf, scales, scale_bias):
    on the device path that is Ns floats read back once per call, after
    prepare and before the first iteration; with check_every=None it is the
    only read-back, and nothing is read back inside the minor cycle.
    Returns (residual, model, components, state, planes, cross_psf)."""
    host = isinstance(residual, np.ndarray)
    scales = [float(a) for a in scales]
    if (not scales or scales[0] != 0.0
            or any(b <= a for a, b in zip(scales, scales[1:]))):
        raise ValueError("scales must be ascending, distinct and start at 0")
    taps = ms_scale_taps(scales)
    if (planes is None) != (cross_psf is None):
        raise ValueError("give planes and cross_psf together")
    if planes is None:
        planes, cross_psf = ms_prepare(residual, psf, taps, stream=stream)
    if host:
        weight, inv_peak = ms_weights(cross_psf, scales, scale_bias)
    else:
        with _on_stream(stream):
            weight, inv_peak = ms_weights(cross_psf, scales, scale_bias)
    _, model, components, state = ms_clean(
        planes, cross_psf, taps, weight, inv_peak, model=model, mask=mask,
        gain=gain, threshold=threshold, cycle_fraction=cycle_fraction,
        max_components=max_components, nr_iterations=nr_iterations,
        components=components, state=state, check_every=check_every,
        stream=stream)
    if host:
        residual[...] = planes[0]
    else:
        with _on_stream(stream):
            residual.copy_(planes[0])
    return residual, model, components, state, planes, cross_psf


# ---------------------------------------------------------------------------
# Restore (idg_beam_* / idg_restore / idg_restore_launch; not
# in the reference): model and residual -> the restored image.  The beam and
# its taps are made on the host; numpy planes take the host entry, torch CUDA
# tensors the _launch entry (asynchronous); the same bytes either way.
#   ... -> clean -> beam_fit(psf) -> restore(model, residual, beam=beam)
# ---------------------------------------------------------------------------
Beam = collections.namedtuple("Beam", "a b c major minor pa")
Beam.__doc__ = """The clean beam exp(-(a dx^2 + 2 b dx dy + c dy^2)) (idg_beam_t):
major >= minor are its FWHMs in pixels, pa the major axis' angle from +x
towards +y in (-pi/2, pi/2]."""


def _beam_struct(beam=None):
    b = BeamStruct()
    b.struct_size = ctypes.sizeof(BeamStruct)
    if beam is not None:
        b.a, b.b, b.c, b.major, b.minor, b.pa = (float(v) for v in beam)
    return b, ctypes.cast(ctypes.pointer(b), ctypes.c_void_p)


def _beam_of(b):
    return Beam(b.a, b.b, b.c, b.major, b.minor, b.pa)


def beam_from_axes(major, minor, pa=0.0):
    """The Beam with FWHMs major >= minor > 0 (pixels) and its major axis at
    angle pa (radians, from +x towards +y)."""
    b, bp = _beam_struct()
    _check(lib.idg_beam_from_axes(float(major), float(minor), float(pa), bp),
           "beam_from_axes")
    return _beam_of(b)


def beam_fit(psf, level=0.5):
    """The Beam fitted to the main lobe of psf (float32 [Gp, Gp], centre
    (Gp // 2, Gp // 2)): the pixels at or above level * the centre that are
    4-connected to it, within 32 pixels (idg_beam_fit; host only, in
    doubles).  numpy, or a CUDA tensor: then the centre window of at most
    65 x 65 floats is copied to the host, which synchronises with the current
    stream."""
    Gp = _square(psf, "psf")
    if not isinstance(psf, np.ndarray):
        import torch
        _dev_ptr(psf, "psf", torch.float32)
        # (the window's centre is at (size // 2, size // 2) again: Gp // 2
        # has as many pixels after it as before it, or one fewer)
        c = Gp // 2
        lo, hi = max(c - 32, 0), min(c + 33, Gp)
        psf = psf[lo:hi, lo:hi].cpu().numpy()
    psf = np.ascontiguousarray(psf)
    b, bp = _beam_struct()
    _check(lib.idg_beam_fit(psf.shape[0], _np_ptr(psf, np.float32, "psf"),
                            float(level), bp), "beam_fit")
    return _beam_of(b)


def beam_radius(beam, cutoff=1e-6):
    """The largest integer distance along the major axis at which the beam is
    still >= cutoff (idg_beam_radius; at most 32)."""
    b, bp = _beam_struct(beam)
    r = lib.idg_beam_radius(bp, float(cutoff))
    if r < 0:
        raise IdgError(r, "beam_radius")
    return r


def beam_taps(beam, radius=None, cutoff=1e-6):
    """The beam on the pixels within `radius` (None: beam_radius(beam,
    cutoff)): float32 [2R + 1, 2R + 1] numpy, the centre 1 (idg_beam_taps)."""
    if radius is None:
        radius = beam_radius(beam, cutoff)
    b, bp = _beam_struct(beam)
    side = 2 * max(int(radius), 0) + 1
    taps = np.empty((side, side), np.float32)
    _check(lib.idg_beam_taps(bp, int(radius), _np_ptr(taps, np.float32,
                                                      "taps", True)),
           "beam_taps")
    return taps


def _restore_params(G, R):
    p = RestoreParamsStruct()
    p.struct_size = ctypes.sizeof(RestoreParamsStruct)
    p.grid_size, p.radius = G, R
    return p, ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)


def restore(model, residual=None, taps=None, beam=None, out=None,
            stream=None):
    """The restored image (idg_restore / idg_restore_launch): `model`
    convolved with the clean beam, plus `residual` (None: none).  All planes
    float32 [G, G].  Give the beam as taps (float32 [2R + 1, 2R + 1], R <= 32,
    as beam_taps makes them; numpy for numpy planes, a CUDA tensor for CUDA
    planes) or as beam= (a Beam: its taps at the default cutoff are built on
    the host and, for CUDA planes, uploaded on `stream`).  out: the plane to
    write, None for a new one; it may be `residual` itself, and no other
    overlap of the buffers is allowed.  Only the non-zero model pixels cost
    anything beyond one pass over the planes.  Returns out."""
    host = isinstance(model, np.ndarray)
    G = _square(model, "model")
    if (taps is None) == (beam is None):
        raise ValueError("give one of taps and beam")
    if beam is not None:
        taps = beam_taps(beam)
        if not host:
            import torch
            with _on_stream(stream):
                taps = torch.from_numpy(taps).to(model.device,
                                                 non_blocking=True)
    side = _square(taps, "taps")
    if side % 2 != 1:
        raise ValueError("taps must be [2R + 1, 2R + 1]")
    R = side // 2
    if residual is not None and tuple(residual.shape) != (G, G):
        raise ValueError("residual must be [G][G]")
    if out is not None and tuple(out.shape) != (G, G):
        raise ValueError("out must be [G][G]")
    p, pp = _restore_params(G, R)
    if host:
        if out is None:
            out = np.empty((G, G), np.float32)
        _check(lib.idg_restore(
            pp, _np_ptr(model, np.float32, "model"),
            None if residual is None else _np_ptr(residual, np.float32,
                                                  "residual"),
            _np_ptr(taps, np.float32, "taps"),
            _np_ptr(out, np.float32, "out", True)), "restore")
        return out
    import torch
    if out is None:
        with _on_stream(stream):
            out = torch.empty((G, G), dtype=torch.float32,
                              device=model.device)
    _check(lib.idg_restore_launch(
        pp, _dev_ptr(model, "model", torch.float32),
        None if residual is None else _dev_ptr(residual, "residual",
                                               torch.float32),
        _dev_ptr(taps, "taps", torch.float32),
        _dev_ptr(out, "out", torch.float32), _stream_handle(stream)),
        "restore")
    return out


# ---------------------------------------------------------------------------
# Perf entries, device info, work model
# ---------------------------------------------------------------------------
def p_run_gridder():
    """hip::p_run_gridder: env-configured perf run; returns ms per launch."""
    ms = lib.idg_p_run_gridder()
    if ms < 0:
        raise IdgError(-1, "p_run_gridder")
    return ms


def p_run_degridder():
    ms = lib.idg_p_run_degridder()
    if ms < 0:
        raise IdgError(-1, "p_run_degridder")
    return ms


def device_name():
    buf = ctypes.create_string_buffer(256)
    n = lib.idg_get_device_name(buf, 256)
    if n < 0:
        raise IdgError(n, "get_device_name")
    return buf.value.decode()


def kernel_name(direction, subgrid_size, nr_channels, options=None):
    d = {"gridder": 0, "degridder": 1}.get(direction, direction)
    keep, optr = _opts_ptr(options)
    name = lib.idg_kernel_name_opts(d, subgrid_size, nr_channels, optr)
    if name is None:
        raise IdgError(-1, "kernel_name")
    return name.decode()


PRECISION_BITS = {1: "reduction tail on every phasor",
                  2: "blocked summation (f32 master every 16 fills)",
                  4: "reduction tail on one channel per quad"}


def precision_options(direction, subgrid_size, nr_channels, options=None):
    """The selected kernels' precision options (include/idg_mi355x.h
    idg_precision_options): (bits, description)."""
    d = {"gridder": 0, "degridder": 1}.get(direction, direction)
    keep, optr = _opts_ptr(options)
    bits = int(lib.idg_precision_options_opts(d, subgrid_size, nr_channels,
                                              optr))
    if bits < 0:
        raise IdgError(bits, "precision_options")
    desc = [v for k, v in PRECISION_BITS.items() if bits & k]
    return bits, "; ".join(desc) if desc else "none"


def flops_gridder(nr_channels, nr_timesteps, nr_subgrids, subgrid_size,
                  nr_correlations=NR_CORRELATIONS):
    """Reference work model (app/common/common.cpp:100-129); nr_timesteps is
    the TOTAL number of timesteps, as the reference passes it."""
    return lib.idg_flops_gridder(nr_channels, nr_timesteps, nr_subgrids,
                                 subgrid_size, nr_correlations)


def bytes_gridder(nr_channels, nr_timesteps, nr_subgrids, subgrid_size,
                  nr_correlations=NR_CORRELATIONS):
    return lib.idg_bytes_gridder(nr_channels, nr_timesteps, nr_subgrids,
                                 subgrid_size, nr_correlations)


def abi_version():
    return lib.idg_abi_version()


def release_workspaces(stream=None, all_streams=False):
    """Free the device workspaces the launch entries cache for `stream` (a
    torch stream; None = the current stream) on the current device, or for
    every stream with all_streams=True (include/idg_mi355x.h
    idg_release_workspaces).  The stream must be idle: call it before
    dropping a stream the entries have used."""
    import torch
    if all_streams:
        handle = ctypes.c_void_p(None)
        # every stream's queued launches finished before their slots go
        torch.cuda.synchronize()
    else:
        handle = _stream_handle(stream)
        (stream or torch.cuda.current_stream()).synchronize()
    _check(lib.idg_release_workspaces(handle, 1 if all_streams else 0),
           "idg_release_workspaces")
