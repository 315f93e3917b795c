"""The restore step's time per call, measured, not gated:
G = 1024, 2048, 4096 with a round beam of FWHM 4 pixels (R = 8 at the default
cutoff), each with a model of 1,000 random components and with a model whose
every pixel is non-zero.

  restore   idg_amd.restore as shipped (taps already on the device)
  conv2d    torch.nn.functional.conv2d of the model with the same taps
            (flipped: conv2d correlates), padding R, plus the residual, in the
            same process
  fft       the FFT route in the same process: irfft2(rfft2(model) *
            rfft2(beam)) + residual at size G x G, the beam's transform made
            once outside the timed window (so the route wraps around at the
            image's edge, which restore and conv2d do not)

each beside its floor: 12 bytes per pixel (model and residual read, restored
written) over the 8 TB/s the bench line uses.

HIP events around windows of CALLS calls; REPS windows of each form taking
turns after a warm-up window; median, min and max per call.  The device's
bytes are checked against the host entry's at G = 1024, both models, before
anything is timed, and conv2d and fft against them to their float32 rounding.

    python tools/debug/restore_rate.py [--out profiles/restore/rate.json]
                                       [--reps 7] [--calls 20]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "ska-sdp-idg-bench_amd"))

HBM_PEAK_GBS = 8000.0     # as bench.py
SIZES = [1024, 2048, 4096]
FWHM = 4.0
COMPONENTS = 1000


def stats(us):
    return {"median": round(float(np.median(us)), 3),
            "min": round(float(min(us)), 3), "max": round(float(max(us)), 3)}


def models(G, seed=1):
    rng = np.random.default_rng(seed)
    sparse = np.zeros((G, G), np.float32)
    ys, xs = rng.integers(0, G, (2, COMPONENTS))
    sparse[ys, xs] = rng.uniform(0.1, 10.0, COMPONENTS)
    dense = rng.uniform(0.5, 1.5, (G, G)).astype(np.float32)
    residual = (0.01 * rng.normal(size=(G, G))).astype(np.float32)
    return {"sparse": sparse, "dense": dense}, residual


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "restore",
                                                  "rate.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as nnf
    import idg_amd
    assert torch.cuda.is_available(), "needs a HIP device"
    N = args.calls
    dev = torch.device("cuda")
    beam = idg_amd.beam_from_axes(FWHM, FWHM, 0.0)
    taps0 = idg_amd.beam_taps(beam)
    R = taps0.shape[0] // 2
    taps = torch.from_numpy(taps0).to(dev)
    weight = torch.from_numpy(taps0[::-1, ::-1].copy()).to(dev)[None, None]

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / N      # us per call

    rows = []
    checked = {}
    for G in SIZES:
        planes, res0 = models(G)
        residual = torch.from_numpy(res0).to(dev)
        out = torch.empty_like(residual)
        kernel = torch.zeros((G, G), dtype=torch.float32, device=dev)
        kernel[:2 * R + 1, :2 * R + 1] = taps
        kernel_f = torch.fft.rfft2(torch.roll(kernel, (-R, -R), (0, 1)))
        floor_us = 12.0 * G * G / (HBM_PEAK_GBS * 1e9) * 1e6
        for kind, m0 in planes.items():
            model = torch.from_numpy(m0).to(dev)

            def restore():
                idg_amd.restore(model, residual, taps=taps, out=out)

            def conv2d():
                return nnf.conv2d(model[None, None], weight,
                                  padding=R)[0, 0] + residual

            def fft():
                return torch.fft.irfft2(torch.fft.rfft2(model) * kernel_f,
                                        s=(G, G)) + residual

            restore()
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            if G == SIZES[0]:
                host = idg_amd.restore(m0, res0, taps=taps0)
                inner = (slice(R, G - R),) * 2     # (the FFT route wraps)
                checked[kind] = {
                    "grid_size": G,
                    "bytes_equal_host": got.tobytes() == host.tobytes(),
                    "conv2d_max_abs": float(np.abs(
                        conv2d().cpu().numpy() - host).max()),
                    "fft_max_abs_inside": float(np.abs(
                        fft().cpu().numpy() - host)[inner].max()),
                    "restored_max_abs": float(np.abs(host).max())}
                assert checked[kind]["bytes_equal_host"], checked
            forms = [("restore", restore), ("conv2d", conv2d), ("fft", fft)]
            for _, fn in forms:
                timed(fn)
            us = {name: [] for name, _ in forms}
            for _ in range(args.reps):
                for name, fn in forms:
                    us[name].append(timed(fn))
            sources = int(np.count_nonzero(m0))
            row = {"grid_size": G, "radius": R, "model": kind,
                   "sources": sources,
                   "hbm_floor_us": round(floor_us, 3),
                   "restore_us": stats(us["restore"]),
                   "conv2d_us": stats(us["conv2d"]),
                   "fft_us": stats(us["fft"])}
            row["restore_over_floor"] = round(
                row["restore_us"]["median"] / floor_us, 2)
            if kind == "dense":
                # multiply-adds inside the image (edges clipped)
                reach = np.minimum(np.arange(G) + R, G - 1) - np.maximum(
                    np.arange(G) - R, 0) + 1
                macs = float(reach.sum()) ** 2
                row["multiply_adds"] = macs
                row["restore_ps_per_multiply_add"] = round(
                    row["restore_us"]["median"] * 1e6 / macs, 3)
            print(json.dumps(row), flush=True)
            rows.append(row)

    result = {
        "device": idg_amd.device_name(), "reps": args.reps,
        "calls_per_window": N, "beam_fwhm_pixels": FWHM, "radius": R,
        "timing": "HIP events around calls_per_window calls, us per call; "
                  "the forms take turns after a warm-up window each",
        "hbm_peak_gbs": HBM_PEAK_GBS,
        "floor": "12 bytes per pixel (model and residual read, restored "
                 "written)",
        "conv2d": "torch.nn.functional.conv2d with the flipped taps, padding "
                  "R, plus the residual (two kernels and a temporary)",
        "fft": "irfft2(rfft2(model) * rfft2(beam)) + residual at G x G; the "
               "beam's transform is made once, untimed; wraps around at the "
               "edges",
        "checked": checked,
        "sizes": rows,
    }
    if args.out == "-":
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
