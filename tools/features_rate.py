#!/usr/bin/env python3
"""Rate of the feature kernel (pathed_hip_render_features_device, all four buffers) beside the beauty render of the same
samples, on C2 (Cornell box, <= 64 triangles), C4 (teapot) and C5 (the 5.2 M-triangle stand-in), at 64 and 1 024 spp.
One process; every call is timed with a HIP event pair on the call's stream, after a short warm-up call of each kind.
On the BVH scenes the beauty pass traces the same camera ray and more, so a feature pass slower than the beauty pass there is a
defect; the all-triangles kernels of C2 never walk the tree the feature kernel walks, there the ratio is only reported.
Usage: features_rate.py [--scenes C2,C4,C5] [--spp 64,1024] [--dragon 9] [--log profiles/features_rate.log]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {
    "C2": ("scenes/cornell.json", 1024, 1024),
    "C4": ("scenes/teapot.json", 1024, 1024),
    "C5": ("scenes/dragon-standin.json", 1920, 1080),
}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--scenes", default="C2,C4,C5")
    parser.add_argument("--spp", default="64,1024")
    parser.add_argument("--dragon", type=int, default=9)
    parser.add_argument("--log", default=os.path.join(ROOT, "profiles", "features_rate.log"))
    args = parser.parse_args()
    names = args.scenes.split(",")
    if "C5" in names:   # (a child process, before this one's first GPU call)
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_assets.py"), "--dragon", str(args.dragon)], check=True, stdout=subprocess.DEVNULL)

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
    for name in names:
        path, width, height = SCENES[name]
        scene = LoadedScene(path, width, height)
        gpu = HipScene(scene.desc, device=0)
        beauty = torch.zeros((height, width, 3), dtype=torch.float32, device="cuda")
        sums = {"albedo": torch.zeros((height, width, 3), dtype=torch.float32, device="cuda"), "normal": torch.zeros((height, width, 3), dtype=torch.float32, device="cuda"),
                "depth": torch.zeros((height, width), dtype=torch.float32, device="cuda"), "hits": torch.zeros((height, width), dtype=torch.float32, device="cuda")}
        pointers = {k: v.data_ptr() for k, v in sums.items()}
        gpu.render_device(1, 0, 8, 0, 10, beauty.data_ptr(), stream)
        gpu.render_features_device(1, 0, 8, stream=stream, **pointers)
        for spp in [int(v) for v in args.spp.split(",")]:
            samples = width * height * spp / 1e6
            feature_seconds = min(timed(lambda: gpu.render_features_device(1, 0, spp, stream=stream, **pointers)) for _ in range(2))
            beauty_seconds = min(timed(lambda: gpu.render_device(1, 0, spp, 0, 10, beauty.data_ptr(), stream)) for _ in range(2))
            feature_rate, beauty_rate = samples / feature_seconds, samples / beauty_seconds
            verdict = ""
            if name != "C2" and feature_rate < beauty_rate:
                verdict = "   DEFECT: the feature pass is slower than the beauty pass, which traces the same ray and more"
            lines.append("%s %s %dx%d x %d spp: features %.0f Msamples/s, beauty (bounces 0..10) %.0f Msamples/s, features / beauty %.2f%s" % (
                name, path, width, height, spp, feature_rate, beauty_rate, feature_rate / beauty_rate, verdict))
            print(lines[-1], flush=True)
        covered = float((sums["hits"] > 0).float().mean().item())
        lines.append("%s: %.1f %% of the pixels are covered" % (name, 100.0 * covered))
        print(lines[-1], flush=True)
        gpu.close()
    with open(args.log, "w") as handle:
        handle.write("tools/features_rate.py --scenes %s --spp %s (best of two timed calls each, HIP events)\n" % (args.scenes, args.spp))
        handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
