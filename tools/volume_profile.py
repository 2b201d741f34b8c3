"""Waves and lanes per region of k_path_volume / k_path_scatter (needs a -DPATHED_EXPERIMENTS=1 -DPATHED_SHADE_PROFILE build of the library):
PATHED_HIP_LIB=pathed_amd/lib/libpathed_hip_profile.so PATHED_VOLUME_PROFILE=1 python tools/volume_profile.py [scene] [w h spp] [integrator]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.chdir(ROOT)
from pathed_amd.integrator import HipScene
from pathed_amd.scene import LoadedScene
path = sys.argv[1] if len(sys.argv) > 1 else "scenes/cornell-medium.json"
w, h, spp = (int(v) for v in sys.argv[2:5]) if len(sys.argv) > 4 else (512, 512, 32)
scene = LoadedScene(path, w, h)
integrator = sys.argv[5] if len(sys.argv) > 5 else "VolumePathTracer"
gpu = HipScene(scene.desc, device=0, grids=scene.grids)
gpu.set_integrator(integrator)
gpu.render(1, 0, 4, 0, 10)
gpu.reset_stats()
gpu.render(1, 4, spp, 0, 10)
print(path, w, h, spp, integrator, flush=True)
gpu.stats()
