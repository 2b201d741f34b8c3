#!/usr/bin/env python3
"""Rate of pathed_hip_render_moments_device (radiance sums + per-channel square sums) beside pathed_hip_render_device on the
same scene and samples: C2 (Cornell box, the fused kernel) and C4 (teapot: the wavefront at this call size, and the wave
path kernel forced).  One process, the two calls alternating; every call is timed with a HIP event pair on the call's stream after a
warm-up call of each kind; the median of the timed calls is reported.
Usage: moments_rate.py [--scenes C2,C4] [--spp 256] [--repeats 5] [--log profiles/moments_rate.log]"""
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


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--scenes", default="C2,C4,C4-wave")
    parser.add_argument("--spp", type=int, default=256)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--log", default=os.path.join(ROOT, "profiles", "moments_rate.log"))
    args = parser.parse_args()

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
        plain, sums, squares = (torch.zeros((height, width, 3), dtype=torch.float32, device="cuda") for _ in range(3))
        render = lambda: gpu.render_device(1, 0, args.spp, 0, 10, plain.data_ptr(), stream)
        moments = lambda: gpu.render_moments_device(1, 0, args.spp, 0, 10, sums.data_ptr(), squares.data_ptr(), stream)
        render()
        moments()
        seconds = {"render": [], "moments": []}
        for _ in range(args.repeats):
            seconds["render"].append(timed(render))
            seconds["moments"].append(timed(moments))
        samples = width * height * args.spp / 1e6
        median = {key: sorted(values)[len(values) // 2] for key, values in seconds.items()}
        lines.append("%s %s %dx%d x %d spp (path kernel %d): render %.0f Msamples/s, with moments %.0f Msamples/s, moments / render %.3f" % (
            name, path, width, height, args.spp, gpu.stats()["path_kernel"], samples / median["render"], samples / median["moments"],
            median["render"] / median["moments"]))
        print(lines[-1], flush=True)
        assert torch.equal(plain, sums)   # the same radiance sums, continued over the same calls
        gpu.close()
    with open(args.log, "w") as handle:
        handle.write("tools/moments_rate.py --scenes %s --spp %d --repeats %d (median of the timed calls, HIP events)\n" % (args.scenes, args.spp, args.repeats))
        handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
