#!/usr/bin/env python3
"""Rate and memory of instanced scenes, alternating in one process:

  (a) a scene that fits both ways: 64 placements of an 80 K-triangle stand-in mesh over a floor under an emitter,
      1024^2 x 64 spp, INSTANCED (k_trace_instanced / k_shade_instanced) against FLATTENED on the wavefront
      (shade_kernel per-slot), Msamples/s and the device bytes of the geometry of both
  (b) jobs/instances-field.json: Msamples/s, its bytes, and the bytes its flattened form would need

    tools/instances_rate.py [--spp 64] [--repeats 3] [--size 1024]

Bytes: 128 per node and 48 per leaf triangle (PathedStats.bvh_bytes), 160 of shading records per stored triangle, 112 per
placement.  The flattened form of (b) is not built: its triangle count is known, its node count is taken as that of (a)'s
flattened tree per triangle.
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

from pathed_amd import flatten_instances  # noqa: E402
from pathed_amd.integrator import HipScene  # noqa: E402
from pathed_amd.scene import LoadedScene  # noqa: E402


def stand_in(subdivisions):
    from instances_scene import icosphere
    return icosphere((0.0, 1.2, 0.0), 1.0, subdivisions)


def scene_a(size, subdivisions=6, side=8):
    from scene_builder import BuiltScene
    scene = BuiltScene(size, size, origin=(0.0, 14.0, 26.0), target=(0.0, 0.5, 0.0), fov_degrees=40.0)
    floor = scene.material(diffuse=(0.6, 0.6, 0.55))
    light = scene.material(diffuse=(0.0, 0.0, 0.0), emit=(20.0, 19.0, 17.0))
    skin = scene.material(diffuse=(0.7, 0.35, 0.25))
    scene.quad([(-20, 0, -20), (-20, 0, 20), (20, 0, 20), (20, 0, -20)], floor)
    scene.quad([(-6, 16, -6), (6, 16, -6), (6, 16, 6), (-6, 16, 6)], light)
    positions, faces, normals, uvs = stand_in(subdivisions)
    scene.mesh(positions, faces, skin, normals=normals, uvs=uvs)
    pointer = scene.finish()
    placements = []
    for k in range(side * side):
        row, col = divmod(k, side)
        angle = np.radians(23.0 * k)
        c, s = np.cos(angle), np.sin(angle)
        linear = (0.8 + 0.05 * (k % 5)) * np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        transform = np.zeros((3, 4))
        transform[:, :3] = linear
        transform[:, 3] = ((col - (side - 1) / 2) * 3.0, 0.0, (row - (side - 1) / 2) * 3.0)
        placements.append((0, transform.astype(np.float32).reshape(12)))
    return scene, pointer, [(2, 1)], placements


def geometry_bytes(gpu, stored_triangles, placements):
    return int(gpu.stats()["bvh_bytes"]) + 160 * stored_triangles + 112 * placements


def rate(gpu, spp, last_bounce, accum):
    accum[:] = 0
    start = time.perf_counter()
    gpu.render(1, 0, spp, 0, last_bounce, accum)
    seconds = time.perf_counter() - start
    return gpu.width * gpu.height * spp / seconds / 1e6, float(accum.astype(np.float64).sum())


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--spp", type=int, default=64)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--size", type=int, default=1024)
    args = parser.parse_args()

    built, pointer, prototypes, placements = scene_a(args.size)
    flat = flatten_instances(pointer, prototypes, placements)
    stored, flat_triangles = int(built.desc.n_triangles), int(flat.desc.contents.n_triangles)
    instanced_gpu = HipScene(pointer, device=0, prototypes=prototypes, instances=placements)
    flat_gpu = HipScene(flat.desc, device=0, shade_kernel="per-slot")
    job = json.load(open(os.path.join(ROOT, "jobs", "instances-field.json")))
    field = LoadedScene(job["scene"], job["width"], job["height"])
    field_gpu = HipScene(field.desc, device=0, prototypes=field.prototypes, instances=field.instances)
    field_stored = int(field.desc.contents.n_triangles)
    field_flat = sum(field.desc.contents.geoms[g].count for g in range(field.prototypes[0][0]))
    for prototype, _ in field.instances:
        first, count = field.prototypes[prototype]
        field_flat += sum(field.desc.contents.geoms[first + g].count for g in range(count))

    accum = np.zeros((args.size, args.size, 3), dtype=np.float32)
    field_accum = np.zeros((job["height"], job["width"], 3), dtype=np.float32)
    results = {"a-instanced": [], "a-flattened": [], "b-field": []}
    sums = {}
    for gpu, image in ((instanced_gpu, accum), (flat_gpu, accum), (field_gpu, field_accum)):   # warm-up: allocations, first launches
        gpu.render(1, 0, 1, 0, 2, image)
    for _ in range(args.repeats):
        for name, gpu, image, bounces in (("a-instanced", instanced_gpu, accum, 4), ("a-flattened", flat_gpu, accum, 4),
                                          ("b-field", field_gpu, field_accum, job["lastBounce"])):
            value, total = rate(gpu, args.spp, bounces, image)
            results[name].append(value)
            sums[name] = total
    flat_bytes = geometry_bytes(flat_gpu, flat_triangles, 0)
    nodes_per_triangle = (int(flat_gpu.stats()["bvh_bytes"]) - 48 * flat_triangles) / 128.0 / flat_triangles
    report = {
        "a": {"placements": len(placements), "stored_triangles": stored, "flattened_triangles": flat_triangles,
              "instanced_msamples": results["a-instanced"], "flattened_msamples": results["a-flattened"],
              "instanced_bytes": geometry_bytes(instanced_gpu, stored, len(placements)), "flattened_bytes": flat_bytes,
              "image_sums": [sums["a-instanced"], sums["a-flattened"]], "path_kernels": [instanced_gpu.stats()["path_kernel"], flat_gpu.stats()["path_kernel"]]},
        "b": {"placements": len(field.instances), "stored_triangles": field_stored, "flattened_triangles": field_flat,
              "msamples": results["b-field"], "bytes": geometry_bytes(field_gpu, field_stored, len(field.instances)),
              "flattened_bytes_estimate": int(field_flat * (48 + 160 + 128 * nodes_per_triangle))},
    }
    for key, value in report.items():
        print("%s %s" % (key, json.dumps(value)))
    for name, values in results.items():
        print("%-12s median %.1f Msamples/s  (%s)" % (name, float(np.median(values)), ", ".join("%.1f" % v for v in values)))


if __name__ == "__main__":
    main()
