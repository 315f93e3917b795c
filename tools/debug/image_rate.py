"""The grid <-> image steps' time, measured, not gated:

  grid_fft       idg_amd.grid_fft_launch, 4 planes, G = 1024 / 2048 / 4096
  grid_to_image  idg_amd.grid_to_image   } W = 1 (w_step 0) and W = 4, with a
  image_to_grid  idg_amd.image_to_grid   } correction, same G

each beside
  * its HBM floor: the bytes a two-pass transform must move (every pass
    reads and writes the planes it transforms; for the two steps, with the
    image-side work fused in: three passes over the grid, the image and the
    correction once) over the peak the bench line uses (8 TB/s);
  * torch.fft.fft2 on the device for the same planes -- for the two
    steps with the separate passes a caller of a library FFT needs (centre
    flips, w phasor, layer sum / broadcast, correction), their tables
    precomputed and not timed.

HIP events around windows of LAUNCHES back-to-back calls after a warm-up of
every shape; ours and torch's windows alternate, REPS of each; median, min
and max per launch.  The two steps' outputs are compared with torch's before
anything is timed.

    python tools/debug/image_rate.py [--out profiles/image/rate.json]
                                     [--sizes 1024,2048,4096] [--reps 7]
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
IMAGE_SIZE, W_STEP = 0.125, 500.0
LAUNCHES = 5


def stats(ms):
    return {"median": round(float(np.median(ms)), 5),
            "min": round(float(min(ms)), 5), "max": round(float(max(ms)), 5)}


def window(fn, reset=None):
    import torch
    if reset is not None:
        reset()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


def interleaved(ours, theirs, reps, reset=None):
    for fn in (ours, theirs):           # warm-up of both
        window(fn, reset)
    a, b = [], []
    for _ in range(reps):
        a.append(window(ours, reset))
        b.append(window(theirs, reset))
    return stats(a), stats(b)


def floor_ms(nbytes):
    return round(nbytes / (HBM_PEAK_GBS * 1e9) * 1e3, 5)


def tables(G, W, w_step, dev):
    """flip [G, G], w phasors [W, 1, G, G] complex64 (exp(+i ...)), from
    float64."""
    import torch
    s = 1.0 - 2.0 * (torch.arange(G, device=dev) % 2).double()
    l = (torch.arange(G, device=dev).double() - G // 2) * (IMAGE_SIZE / G)
    tmp = l[:, None] ** 2 + l[None, :] ** 2
    n = tmp / (1 + torch.sqrt(1 - tmp))
    z = torch.arange(W, device=dev).double() + 0.5
    ph = torch.polar(torch.ones_like(n)[None].expand(W, G, G).contiguous(),
                     2 * np.pi * w_step * z[:, None, None] * n[None])
    return (s[:, None] * s[None, :]).float(), ph.to(torch.complex64)[:, None]


def measure(idg, G, reps):
    import torch
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(G)
    out = {}
    plane_bytes = G * G * 8

    # ---- the plain transform, 4 planes
    x = torch.randn((4, G, G, 2), device=dev, generator=gen)
    work = x.clone()
    xc = torch.view_as_complex(x)
    idg.grid_fft_launch(work, -1)
    err = (torch.view_as_complex(work) - torch.fft.fft2(xc)).abs().max() / \
        torch.fft.fft2(xc).abs().max()
    ours, theirs = interleaved(
        lambda: idg.grid_fft_launch(work, -1, 1.0 / G),
        lambda: torch.fft.fft2(xc), reps, lambda: work.copy_(x))
    out["grid_fft_4_planes"] = {
        "ms": ours, "torch_fft2_ms": theirs,
        "hbm_floor_ms": floor_ms(2 * 2 * 4 * plane_bytes),
        "floor": "2 passes x (read + write) x 4 planes",
        "max_abs_diff_to_torch_over_peak": float(err)}
    del work, xc, x

    # ---- grid_to_image / image_to_grid
    corr = torch.rand((G, G), device=dev, generator=gen) + 0.5
    for W, w_step in ((1, 0.0), (4, W_STEP)):
        flip, ph = tables(G, W, w_step, dev)
        grid0 = torch.randn((W, 4, G, G, 2), device=dev, generator=gen)
        grid = grid0.clone()
        image = torch.randn((4, G, G, 2), device=dev, generator=gen)
        gc, ic_ = torch.view_as_complex(grid0), torch.view_as_complex(image)
        nbytes = (3 * W * 4 + 4) * plane_bytes + G * G * 4

        def torch_to_image():
            f = torch.fft.fft2(gc * flip) * flip
            return (f * ph.conj()).sum(0) * corr

        def torch_to_grid():
            src = (ic_ * corr * flip)[None] * ph
            return torch.fft.ifft2(src, norm="forward") * flip

        got = torch.view_as_complex(idg.grid_to_image(
            G, IMAGE_SIZE, w_step, grid, nr_w_layers=W, correction=corr))
        want = torch_to_image()
        e1 = float((got - want).abs().max() / want.abs().max())
        got = torch.view_as_complex(idg.image_to_grid(
            G, IMAGE_SIZE, w_step, image, grid, nr_w_layers=W,
            correction=corr))
        want = torch_to_grid()
        e2 = float((got - want).abs().max() / want.abs().max())
        del got, want
        out_img = torch.empty_like(image)
        ours, theirs = interleaved(
            lambda: idg.grid_to_image(G, IMAGE_SIZE, w_step, grid, out_img,
                                      nr_w_layers=W, correction=corr),
            torch_to_image, reps, lambda: grid.copy_(grid0))
        out[f"grid_to_image_W{W}"] = {
            "ms": ours, "torch_fft2_plus_passes_ms": theirs,
            "hbm_floor_ms": floor_ms(nbytes),
            "max_abs_diff_to_torch_over_peak": e1}
        ours, theirs = interleaved(
            lambda: idg.image_to_grid(G, IMAGE_SIZE, w_step, image, grid,
                                      nr_w_layers=W, correction=corr),
            torch_to_grid, reps)
        out[f"image_to_grid_W{W}"] = {
            "ms": ours, "torch_fft2_plus_passes_ms": theirs,
            "hbm_floor_ms": floor_ms(nbytes),
            "max_abs_diff_to_torch_over_peak": e2}
        del grid0, grid, image, flip, ph, out_img
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "image",
                                                  "rate.json"))
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import idg_amd
    assert torch.cuda.is_available(), "needs a HIP device"
    res = {
        "device": idg_amd.device_name(), "reps": args.reps,
        "launches_per_window": LAUNCHES,
        "timing": "HIP events around windows of back-to-back calls, ms per "
                  "call; ours and torch's windows alternate",
        "hbm_peak_gbs": HBM_PEAK_GBS,
        "step_floor": "(3 W x 4 + 4) planes of 8 G^2 bytes + 4 G^2: what a "
                      "transform with the image-side work fused into a pass "
                      "would move; the library's steps make five passes",
        "image_size": IMAGE_SIZE, "w_step_W4": W_STEP,
    }
    for G in (int(s) for s in args.sizes.split(",")):
        res[f"G{G}"] = measure(idg_amd, G, args.reps)
        print(json.dumps({f"G{G}": res[f"G{G}"]}), flush=True)
    if args.out == "-":
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
