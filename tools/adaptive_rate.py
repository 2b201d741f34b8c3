#!/usr/bin/env python3
"""What a pixel list costs: Msamples/s per RENDERED sample of pathed_hip_render_pixels_device over lists that hold 100 %,
50 % (checkerboard), 10 % and 1 % (scattered, a fixed seed) of the image, beside pathed_hip_render_moments_device on the
whole image in the same process: C2 (Cornell box: the moments call runs the fused kernel) and C4 (teapot: the wavefront at
this call size, and the wave path kernel forced).  A list call always runs the wavefront kernels (the line shows each call's
path kernel), so on C2 and C4-wave the ratio compares two kernel organisations, and on C4 the 100 % list runs the same units
as the plain call through one gather: that ratio is the cost of the list itself.  The calls alternate; every call is timed
with a HIP event pair on the call's stream after a warm-up call of each kind; the median of the timed calls is reported.
Usage: adaptive_rate.py [--scenes C2,C4,C4-wave] [--spp 256] [--repeats 5] [--log profiles/adaptive_rate.log]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {
    "C2": ("scenes/cornell.json", 1024, 1024, {}),
    "C4": ("scenes/teapot.json", 1024, 1024, {}),
    "C4-wave": ("scenes/teapot.json", 1024, 1024, {"shade_kernel": "wave"}),
}


def pixel_lists(width, height):
    import numpy as np
    pixels = width * height
    rows, columns = np.divmod(np.arange(pixels), width)
    rng = np.random.default_rng(1)
    return [
        ("100 %", np.arange(pixels, dtype=np.uint32)),
        ("50 % checkerboard", np.flatnonzero((rows + columns) % 2 == 0).astype(np.uint32)),
        ("10 % scattered", np.sort(rng.choice(pixels, pixels // 10, replace=False)).astype(np.uint32)),
        ("1 % scattered", np.sort(rng.choice(pixels, pixels // 100, replace=False)).astype(np.uint32)),
    ]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--scenes", default="C2,C4,C4-wave")
    parser.add_argument("--spp", type=int, default=256)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--log", default=os.path.join(ROOT, "profiles", "adaptive_rate.log"))
    args = parser.parse_args()

    import numpy as np
    import torch
    from pathed_amd.integrator import HipScene
    from pathed_amd.scene import LoadedScene

    stream = torch.cuda.current_stream().cuda_stream

    def timed(call):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    lines = []
    for name in args.scenes.split(","):
        path, width, height, options = SCENES[name]
        scene = LoadedScene(path, width, height)
        gpu = HipScene(scene.desc, device=0, **options)
        sums, squares, list_sums, list_squares = (torch.zeros((height, width, 3), dtype=torch.float32, device="cuda") for _ in range(4))
        counts = torch.zeros((height, width), dtype=torch.int32, device="cuda")
        lists = [(label, torch.from_numpy(entries.view(np.int32)).cuda(), entries.size) for label, entries in pixel_lists(width, height)]
        calls = {"moments": lambda: gpu.render_moments_device(1, 0, args.spp, 0, 10, sums.data_ptr(), squares.data_ptr(), stream)}
        for label, entries, n_list in lists:
            calls[label] = (lambda entries=entries, n_list=n_list: gpu.render_pixels(
                1, 0, args.spp, 0, 10, entries.data_ptr(), n_list, list_sums.data_ptr(), list_squares.data_ptr(), counts.data_ptr(), stream))
        kernels = {}
        for label, call in calls.items():   # warm-up, and which kernel each call runs
            call()
            kernels[label] = gpu.stats()["path_kernel"]
        seconds = {label: [] for label in calls}
        for _ in range(args.repeats):
            for label, call in calls.items():
                seconds[label].append(timed(call))
        median = {label: sorted(values)[len(values) // 2] for label, values in seconds.items()}
        base = width * height * args.spp / 1e6 / median["moments"]
        text = "%s %s %dx%d x %d spp: moments call %.0f Msamples/s (path kernel %d); lists, Msamples/s per rendered sample (ratio to it, path kernel):" % (
            name, path, width, height, args.spp, base, kernels["moments"])
        for label, entries, n_list in lists:
            rate = n_list * args.spp / 1e6 / median[label]
            text += "  %s %.0f (%.3f, %d)" % (label, rate, rate / base, kernels[label])
        lines.append(text)
        print(text, flush=True)
        gpu.close()
    with open(args.log, "w") as handle:
        handle.write("tools/adaptive_rate.py --scenes %s --spp %d --repeats %d (median of the timed calls, HIP events)\n" % (args.scenes, args.spp, args.repeats))
        handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
