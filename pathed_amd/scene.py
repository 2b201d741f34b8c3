"""Scene loading through the C++ host library (reference formats)."""
import ctypes as C

from . import _capi


class LoadedScene:
    """Owns a FlatScene inside libpathed_host.so; `.desc` is a PathedSceneDesc pointer."""

    def __init__(self, scene_path, width, height, asset_root=None):
        self._host = _capi.load_host()
        root = asset_root if asset_root is not None else _capi.REPO_ROOT
        self._handle = self._host.pathed_host_load_scene(scene_path.encode(), width, height, root.encode())
        if not self._handle:
            raise RuntimeError(self._host.pathed_host_last_error().decode())
        self.desc = self._host.pathed_host_scene_desc(self._handle)
        # the scene file's "heterogeneous" media: (medium slot, _capi.PathedGridMedium) pairs for HipScene(..., grids=...); the
        # structs point into this object
        self.grids = []
        for i in range(self._host.pathed_host_scene_grid_count(self._handle)):
            slot = C.c_int(-1)
            grid = self._host.pathed_host_scene_grid(self._handle, i, C.byref(slot))
            self.grids.append((slot.value, grid.contents))
        # media with a "phase" key of type "henyey-greenstein": (medium slot, g) pairs for HipScene(..., phases=...)
        self.phases = []
        for i in range(self._host.pathed_host_scene_phase_count(self._handle)):
            slot, g = C.c_int(-1), C.c_float(0.0)
            self._host.pathed_host_scene_phase(self._handle, i, C.byref(slot), C.byref(g))
            self.phases.append((slot.value, g.value))
        # "instance" / "instanced" models: (prototypes, instances) as HipScene(..., prototypes=, instances=) and
        # pathed_amd.flatten_instances take them -- one level, nesting resolved and emissive faces baked by the loader; None = flat
        self.prototypes, self.instances = None, None
        found = self._host.pathed_host_scene_instances(self._handle)
        if found:
            described = found.contents
            self.prototypes = [(described.prototypes[i].first_geom, described.prototypes[i].n_geoms) for i in range(described.n_prototypes)]
            self.instances = [(described.instances[i].prototype, [float(x) for x in described.instances[i].transform]) for i in range(described.n_instances)]
        # top-level "instanced" models with "transform_close": the placements at shutter time 1, (n, 12) float32 in instance order
        # for HipScene.set_instance_motion (a placement that does not move: its transform again); None = nothing moves
        self.instances_close = None
        close = self._host.pathed_host_scene_instances_close(self._handle) if self.instances else None
        if close:
            import numpy as np
            self.instances_close = np.ctypeslib.as_array(close, shape=(len(self.instances), 12)).astype(np.float32).copy()
        self.width = width
        self.height = height

    def close(self):
        if self._handle:
            self._host.pathed_host_free_scene(self._handle)
            self._handle = None

    def __del__(self):
        self.close()

    @property
    def n_triangles(self):
        return int(self.desc.contents.n_triangles)

    @property
    def n_spheres(self):
        return int(self.desc.contents.n_spheres)

    @property
    def n_materials(self):
        return int(self.desc.contents.n_materials)
