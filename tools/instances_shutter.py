#!/usr/bin/env python3
"""What the shutter over instanced scenes costs (DESIGN.md section 4.6d "Shutter"), the arms alternating in one process, on
jobs/instances-field-motion.json (400 placements, five of them moving) and on the 64-placement scene of
tools/instances_rate.py (64 placements of an 80 K-triangle mesh):

  (a) overhead      the motion kernels with a zero-width shutter [t, t] against the static kernels on a scene CREATED with the
                    placements of time t: the same image, bit for bit -- what the motion variant costs by itself
  (b) open shutter  [0, 1] with ALL placements moving and with a FEW moving (the field: its five; the 64: four)
  (c) host loop     what the shutter replaces: per sample, set_instance_transforms at that sample's time plus a one-sample
                    render (one time per sample index here, so this arm does less than (b): its samples of one index share
                    a time)

    tools/instances_shutter.py [--spp 64] [--repeats 3] [--size 1024] [--log profiles/instances_shutter.log]

Msamples/s are wall-clock over a whole render call (host synchronised), best of --repeats after one warm-up call per arm.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pathed_amd import instances as I  # noqa: E402
from pathed_amd.integrator import HipScene  # noqa: E402
from pathed_amd.scene import LoadedScene  # noqa: E402

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def moved(transforms, which, rng):
    """time-1 transforms: the rows `which` turned about y, lifted and shifted by about a placement's size; the others as they are"""
    out = transforms.copy()
    for k in which:
        m = transforms[k].reshape(3, 4).astype(np.float64)
        angle = rng.uniform(0.5, 2.5)
        c, s = np.cos(angle), np.sin(angle)
        turn = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        scale = np.linalg.norm(m[:, 0])
        close = np.zeros((3, 4))
        close[:, :3] = turn @ m[:, :3]
        close[:, 3] = m[:, 3] + scale * rng.uniform(-2.0, 2.0, 3) * np.array([1.0, 0.5, 1.0]) + np.array([0.0, 1.5 * scale, 0.0])
        out[k] = close.astype(np.float32).reshape(12)
    return out


def rate(render, pixels, spp, repeats):
    render()   # warm-up: allocations, the first launch of every kernel
    best = 0.0
    for _ in range(repeats):
        start = time.perf_counter()
        render()
        best = max(best, pixels * spp / (time.perf_counter() - start) / 1e6)
    return best


def measure(name, desc, prototypes, which, open_transforms, close_all, close_few, few, width, height, spp, last_bounce, repeats):
    pixels = width * height
    make = lambda transforms: HipScene(desc, device=0, prototypes=prototypes, instances=[(int(p), t) for p, t in zip(which, transforms)])
    accum = np.zeros((height, width, 3), dtype=np.float32)

    def full(gpu):
        def render():
            accum[:] = 0
            gpu.render(1, 0, spp, 0, last_bounce, accum)
        return render

    say("## %s: %d placements, %d x %d x %d spp, bounces 0..%d" % (name, len(which), width, height, spp, last_bounce))
    # (a) zero-width shutter against the static kernels on the scene created at that time
    t = 0.5
    halfway = I.interpolate_transforms(open_transforms, close_all, t)
    static = make(halfway)
    frozen = make(open_transforms)
    frozen.set_instance_motion(close_all, shutter=(t, t))
    rates = {"static": [], "frozen": []}
    for _ in range(2):   # alternating
        rates["static"].append(rate(full(static), pixels, spp, repeats))
        static_sum = float(accum.astype(np.float64).sum())
        static_image = accum.copy()
        rates["frozen"].append(rate(full(frozen), pixels, spp, repeats))
        same = np.array_equal(accum.view(np.uint32), static_image.view(np.uint32))
    assert static.stats()["path_kernel"] == 10 and frozen.stats()["path_kernel"] == 11
    say("(a) static kernels at t = %.2f        %8.1f Msamples/s   (runs: %s)" % (t, max(rates["static"]), ", ".join("%.1f" % r for r in rates["static"])))
    say("(a) motion kernels, shutter [t, t]    %8.1f Msamples/s   (runs: %s)   ratio %.3f   same bits: %s   image sum %.6g"
        % (max(rates["frozen"]), ", ".join("%.1f" % r for r in rates["frozen"]), max(rates["frozen"]) / max(rates["static"]), same, static_sum))
    # (b) open shutter, all moving and a few moving
    moving_all, moving_few = make(open_transforms), make(open_transforms)
    ms_all = moving_all.set_instance_motion(close_all)
    ms_few = moving_few.set_instance_motion(close_few)
    open_rates = {"all": [], "few": []}
    for _ in range(2):
        open_rates["all"].append(rate(full(moving_all), pixels, spp, repeats))
        open_rates["few"].append(rate(full(moving_few), pixels, spp, repeats))
    say("(b) open shutter, all %d moving       %8.1f Msamples/s   (runs: %s)   set_instance_motion %.3f ms"
        % (len(which), max(open_rates["all"]), ", ".join("%.1f" % r for r in open_rates["all"]), ms_all))
    say("(b) open shutter, %d moving            %8.1f Msamples/s   (runs: %s)   set_instance_motion %.3f ms"
        % (few, max(open_rates["few"]), ", ".join("%.1f" % r for r in open_rates["few"]), ms_few))
    # (c) the per-sample host loop
    loop = make(open_transforms)
    times = I.sample_time(1, 0, np.arange(spp), 0.0, 1.0)
    steps = [I.interpolate_transforms(open_transforms, close_all, time_k) for time_k in times]

    def host_loop():
        accum[:] = 0
        for sample in range(spp):
            loop.set_instance_transforms(steps[sample])
            loop.render(1, sample, 1, 0, last_bounce, accum)
    loop_rate = rate(host_loop, pixels, spp, max(1, repeats - 1))
    say("(c) host loop, %d x (set_instance_transforms + 1 spp)   %8.1f Msamples/s   (open shutter, all moving: %.2f x)"
        % (spp, loop_rate, max(open_rates["all"]) / loop_rate))
    return same


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--spp", type=int, default=64)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--size", type=int, default=1024)
    parser.add_argument("--log", default=os.path.join(ROOT, "profiles", "instances_shutter.log"))
    args = parser.parse_args()
    say("# tools/instances_shutter.py --spp %d --repeats %d --size %d" % (args.spp, args.repeats, args.size))
    rng = np.random.default_rng(11)
    same = []

    job = json.load(open(os.path.join(ROOT, "jobs", "instances-field-motion.json")))
    field = LoadedScene(job["scene"], job["width"], job["height"])
    which = np.array([p for p, _ in field.instances], dtype=np.int64)
    open_transforms = np.array([t for _, t in field.instances], dtype=np.float32).reshape(-1, 12)
    close_few = field.instances_close
    few = int((close_few.view(np.uint32) != open_transforms.view(np.uint32)).any(axis=1).sum())
    close_all = moved(open_transforms, range(len(which)), rng)
    same.append(measure("instances-field-motion", field.desc, field.prototypes, which, open_transforms, close_all, close_few, few,
                        job["width"], job["height"], args.spp, job["lastBounce"], args.repeats))

    from instances_rate import scene_a
    built, pointer, prototypes, placements = scene_a(args.size)
    which = np.array([p for p, _ in placements], dtype=np.int64)
    open_transforms = np.stack([t for _, t in placements]).astype(np.float32)
    close_all = moved(open_transforms, range(len(which)), rng)
    close_few = moved(open_transforms, [5, 21, 38, 59], rng)
    same.append(measure("64 placements of an 80 K-triangle mesh", pointer, prototypes, which, open_transforms, close_all, close_few, 4,
                        args.size, args.size, args.spp, 4, args.repeats))

    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as handle:
        handle.write("\n".join(LINES) + "\n")
    assert all(same), "a zero-width shutter did not render the static scene's bits"


if __name__ == "__main__":
    main()
