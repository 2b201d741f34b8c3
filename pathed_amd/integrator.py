"""Python mirror of the reference's Integrator plug-in surface for the GPU path.

Reference: include/integrator.h:16-55 (`Integrator::run(image, scene, callback, quit)`),
src/integrator.cpp:19-106 (wave loop, sum -> mean, power-of-two checkpoints) and
src/job.cpp:65-97 (the "integrator" string factory).  The C++ twin of this file is
pathed_amd/host/integrator.{h,cpp}; both sit directly on include/pathed_hip.h.

Everything computed here happens inside libpathed_hip.so; if that library (or a GPU)
is missing the calls raise — there is no CPU fallback in the product path.
"""
import ctypes as C

import numpy as np

from . import _capi


class PathedError(RuntimeError):
    pass


def _check(lib, code, what):
    if code != 0:
        raise PathedError("%s failed (%d): %s" % (what, code, lib.pathed_hip_last_error().decode()))


SEED_RANGE = "an integer in [0, 2^64)"


def _seed(seed):
    """The seed of a render call: an integer in [0, 2^64).  ctypes would wrap -1 to 2^64 - 1 and 2^64 to 0 without a word."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise PathedError("seed must be %s, not %r" % (SEED_RANGE, seed))
    return int(seed)


def measure_bandwidth(gib=2.0, repeats=10):
    """(read GB/s, copy GB/s) of a plain streaming kernel on the current device (pathed_hip_measure_bandwidth)."""
    lib = _capi.load_hip()
    read, copy = C.c_double(0.0), C.c_double(0.0)
    _check(lib, lib.pathed_hip_measure_bandwidth(int(gib * (1 << 30)), int(repeats), C.byref(read), C.byref(copy)),
           "pathed_hip_measure_bandwidth")
    return read.value, copy.value


def measure_valu(waves_per_simd=4, repeats=10):
    """(v_fma_f32, fma + rcp/sqrt mix) wave-instructions per second the device sustains (pathed_hip_measure_valu)."""
    lib = _capi.load_hip()
    fma, mixed = C.c_double(0.0), C.c_double(0.0)
    _check(lib, lib.pathed_hip_measure_valu(int(waves_per_simd), int(repeats), C.byref(fma), C.byref(mixed)),
           "pathed_hip_measure_valu")
    return fma.value, mixed.value


VALU_MODES = ("v_fma_f32 (1 VGPR source)", "6 v_fma_f32 + v_rcp_f32 + v_sqrt_f32", "v_fma_f32 (3 VGPR sources)", "v_pk_fma_f32", "v_mul_lo_u32")


def measure_valu_modes(waves_per_simd=4, repeats=5):
    """wave-instructions per second for each of VALU_MODES (pathed_hip_measure_valu_modes)."""
    lib = _capi.load_hip()
    rates = (C.c_double * 5)()
    _check(lib, lib.pathed_hip_measure_valu_modes(int(waves_per_simd), int(repeats), rates, 5), "pathed_hip_measure_valu_modes")
    return list(rates)


def measure_valu_clocks(waves_per_simd=4, chains=8, repeats=5):
    """v_fma_f32 issue rate with the probe's own clocks (pathed_hip_measure_valu_clocks): a dict with the rate, the shader
    clock the chip ran at, and cycles per instruction."""
    lib = _capi.load_hip()
    out = _capi.PathedValuClocks()
    _check(lib, lib.pathed_hip_measure_valu_clocks(int(waves_per_simd), int(chains), int(repeats), C.byref(out)), "pathed_hip_measure_valu_clocks")
    return {name: getattr(out, name) for name, _ in _capi.PathedValuClocks._fields_}


class HipScene:
    """A scene uploaded to one GPU (PathedScene handle).

    Keyword options map onto PathedSceneOptions (include/pathed_hip.h): stack_rows, pools,
    suspend_lanes, suspend_patience, park_min_cards, max_slots, build_threads, generic_kernels, refittable, wave_max_ksamples,
    wave_stragglers, wave_refill, chunks_per_pass, hybrid_batch, hybrid_ready, local_rays, shade_launches, shade_chain, intersector ("auto" | "bvh"),
    trace_blocks_per_cu, shade_kernel ("auto" | "per-slot" | "staged" | "fused" | "split" | "wave" | "hybrid"), stage_slots,
    unit_order ("auto" | "stripes" | "stripes-tiled" | "tiles"), node_format ("auto" | "wide" | "compressed" | "compressed8"), small_phase1 ("auto" | "valu" | "mfma").  `device=None` keeps the device of an earlier pathed_hip_init.
    `grids`: (medium slot, _capi.PathedGridMedium) pairs set on the created scene (LoadedScene.grids; see set_grid_medium).
    `phases`: (medium slot, g) pairs, Henyey-Greenstein phase functions set on the created scene (LoadedScene.phases; see set_medium_phase).
    `prototypes`, `instances`: instanced geometry (pathed_hip_scene_create_instanced) -- prototypes [(first geom, geoms), ...]
    naming the description's last geoms, instances [(prototype, 12 floats: row-major 3 x 4), ...], or an instances.InstanceSet
    as `instances`; hits then carry virtual primitive ids, those of pathed_amd.flatten_instances of the same arguments.
    """

    BVH_BUILDERS = {"sah": 0, "lbvh": 1, "ploc": 2}  # PATHED_BVH_SAH_HOST / _LBVH_DEVICE / _PLOC_DEVICE

    def __init__(self, desc_pointer, device=None, bvh_builder="sah", grids=(), phases=(), prototypes=None, instances=None, **options):
        self._lib = _capi.load_hip()
        packed = _capi.PathedSceneOptions()
        packed.struct_size = C.sizeof(_capi.PathedSceneOptions)
        packed.device = _capi.DEVICE_CURRENT if device is None else int(device)
        packed.bvh_builder = self.BVH_BUILDERS[bvh_builder] + 1
        intersector = options.pop("intersector", "auto")
        packed.intersector = {"auto": 0, "bvh": 1}[intersector]
        packed.shade_kernel = {"auto": 0, "per-slot": 1, "staged": 2, "fused": 3, "split": 4, "wave": 5, "hybrid": 6}[options.pop("shade_kernel", "auto")]
        packed.node_format = {"auto": 0, "wide": 1, "compressed": 2, "compressed8": 3}[options.pop("node_format", "auto")]
        packed.unit_order = {"auto": 0, "stripes": 1, "stripes-tiled": 2, "tiles": 3}[options.pop("unit_order", "auto")]
        packed.small_phase1 = {"auto": 0, "valu": 1, "mfma": 2}[options.pop("small_phase1", "auto")]
        for name in ("stack_rows", "pools", "suspend_lanes", "suspend_patience", "park_min_cards", "max_slots", "trace_blocks_per_cu", "stage_slots", "build_threads", "generic_kernels", "refittable",
                     "wave_max_ksamples", "wave_stragglers", "wave_refill", "chunks_per_pass", "hybrid_batch", "hybrid_ready", "local_rays", "shade_launches", "shade_chain"):
            if name in options:
                setattr(packed, name, int(options.pop(name)))
        if options:
            raise TypeError("unknown scene options: %s" % sorted(options))
        handle = C.c_void_p()
        if instances is not None or prototypes is not None:
            from .instances import InstanceSet
            self.instance_set = instances if isinstance(instances, InstanceSet) else InstanceSet(prototypes or (), instances or ())
            _check(self._lib, self._lib.pathed_hip_scene_create_instanced(desc_pointer, C.byref(packed), C.byref(self.instance_set.desc), C.byref(handle)),
                   "pathed_hip_scene_create_instanced")
        else:
            _check(self._lib, self._lib.pathed_hip_scene_create_ex(desc_pointer, C.byref(packed), C.byref(handle)),
                   "pathed_hip_scene_create_ex")
        self._handle = handle
        self.device = int(self._lib.pathed_hip_scene_device(handle))
        self.width = int(desc_pointer.contents.camera.width)
        self.height = int(desc_pointer.contents.camera.height)
        for medium_index, grid in grids:   # LoadedScene.grids: the voxel-grid media of the scene file
            self.set_grid_medium(medium_index, grid)
        for medium_index, g in phases:   # LoadedScene.phases: the Henyey-Greenstein media of the scene file
            self.set_medium_phase(medium_index, g)

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.pathed_hip_scene_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, seed, spp_begin, spp_count, start_bounce, last_bounce, accum=None):
        """radianceLookup += ... for samples [spp_begin, spp_begin+spp_count); host buffer (H, W, 3)."""
        if accum is None:
            accum = np.zeros((self.height, self.width, 3), dtype=np.float32)
        assert accum.dtype == np.float32 and accum.flags["C_CONTIGUOUS"] and accum.size == 3 * self.width * self.height
        code = self._lib.pathed_hip_render(
            self._handle, C.c_uint64(_seed(seed)), spp_begin, spp_count, start_bounce, last_bounce,
            accum.ctypes.data_as(C.POINTER(C.c_float)))
        _check(self._lib, code, "pathed_hip_render")
        return accum

    def render_device(self, seed, spp_begin, spp_count, start_bounce, last_bounce, device_pointer, stream=0):
        """Same, into caller-owned device memory (e.g. tensor.data_ptr()) on `stream`."""
        code = self._lib.pathed_hip_render_device(
            self._handle, C.c_uint64(_seed(seed)), spp_begin, spp_count, start_bounce, last_bounce,
            C.c_void_p(device_pointer), C.c_void_p(stream), 1)
        _check(self._lib, code, "pathed_hip_render_device")

    def render_features(self, seed, spp_begin, spp_count, albedo=None, normal=None, depth=None, hits=None):
        """First-hit feature sums of samples [spp_begin, spp_begin + spp_count) (pathed_hip_render_features): albedo and normal
        (H, W, 3), depth and hits (H, W), float32 host arrays the call adds its samples to, one by one in sample order.  With no array given all four are made and
        returned; otherwise only the ones passed are rendered (the others come back None)."""
        if albedo is None and normal is None and depth is None and hits is None:
            albedo = np.zeros((self.height, self.width, 3), dtype=np.float32)
            normal = np.zeros((self.height, self.width, 3), dtype=np.float32)
            depth = np.zeros((self.height, self.width), dtype=np.float32)
            hits = np.zeros((self.height, self.width), dtype=np.float32)
        pointers = []
        for array, channels in ((albedo, 3), (normal, 3), (depth, 1), (hits, 1)):
            if array is None:
                pointers.append(None)
                continue
            assert array.dtype == np.float32 and array.flags["C_CONTIGUOUS"] and array.size == channels * self.width * self.height
            pointers.append(array.ctypes.data_as(C.POINTER(C.c_float)))
        code = self._lib.pathed_hip_render_features(self._handle, C.c_uint64(_seed(seed)), spp_begin, spp_count, *pointers)
        _check(self._lib, code, "pathed_hip_render_features")
        return albedo, normal, depth, hits

    def render_features_device(self, seed, spp_begin, spp_count, albedo=0, normal=0, depth=0, hits=0, stream=0):
        """Same, onto caller-owned device memory (e.g. tensor.data_ptr(); 0 = not wanted) on `stream`: the sums CONTINUE from
        the buffers' contents, in sample order."""
        buffers = _capi.PathedFeatureBuffers(albedo or None, normal or None, depth or None, hits or None)
        code = self._lib.pathed_hip_render_features_device(
            self._handle, C.c_uint64(_seed(seed)), spp_begin, spp_count, C.byref(buffers), C.c_void_p(stream))
        _check(self._lib, code, "pathed_hip_render_features_device")

    def render_moments(self, seed, spp_begin, spp_count, start_bounce, last_bounce, accum=None, squares=None):
        """The radiance sums of samples [spp_begin, spp_begin + spp_count) and, beside them, the per-channel sums of the squared
        sample colours (pathed_hip_render_moments): two float32 host arrays (H, W, 3) the call ADDS to, as `render` does."""
        if accum is None:
            accum = np.zeros((self.height, self.width, 3), dtype=np.float32)
        if squares is None:
            squares = np.zeros((self.height, self.width, 3), dtype=np.float32)
        for array in (accum, squares):
            assert array.dtype == np.float32 and array.flags["C_CONTIGUOUS"] and array.size == 3 * self.width * self.height
        code = self._lib.pathed_hip_render_moments(
            self._handle, C.c_uint64(_seed(seed)), spp_begin, spp_count, start_bounce, last_bounce,
            accum.ctypes.data_as(C.POINTER(C.c_float)), squares.ctypes.data_as(C.POINTER(C.c_float)))
        _check(self._lib, code, "pathed_hip_render_moments")
        return accum, squares

    def render_moments_device(self, seed, spp_begin, spp_count, start_bounce, last_bounce, sum_pointer, squares_pointer, stream=0):
        """Same, onto caller-owned device memory (e.g. tensor.data_ptr()) on `stream`: both sums CONTINUE from the buffers'
        contents in sample order, so any split of [0, n) into calls gives the same floats."""
        code = self._lib.pathed_hip_render_moments_device(
            self._handle, C.c_uint64(_seed(seed)), spp_begin, spp_count, start_bounce, last_bounce,
            C.c_void_p(sum_pointer or None), C.c_void_p(squares_pointer or None), C.c_void_p(stream))
        _check(self._lib, code, "pathed_hip_render_moments_device")

    def device_buffer(self, count, host=None):
        """`count` floats on the scene's device (pathed_hip_accum_alloc), zeroed or filled from `host`; free with free_device_buffer."""
        pointer = C.c_void_p()
        _check(self._lib, self._lib.pathed_hip_accum_alloc(self._handle, int(count), C.byref(pointer)), "pathed_hip_accum_alloc")
        if host is not None:
            host = np.ascontiguousarray(host, dtype=np.float32)
            assert host.size == count
            code = self._lib.pathed_hip_accum_upload(self._handle, pointer, int(count), host.ctypes.data_as(C.POINTER(C.c_float)))
            if code != 0:
                self._lib.pathed_hip_accum_free(self._handle, pointer)
            _check(self._lib, code, "pathed_hip_accum_upload")
        return pointer.value

    def download_device_buffer(self, pointer, out):
        """Copies out.size floats from device memory at `pointer` into the float32 array `out`."""
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
        _check(self._lib, self._lib.pathed_hip_accum_download(self._handle, C.c_void_p(pointer), out.size, out.ctypes.data_as(C.POINTER(C.c_float))),
               "pathed_hip_accum_download")
        return out

    def free_device_buffer(self, pointer):
        if pointer:
            self._lib.pathed_hip_accum_free(self._handle, C.c_void_p(pointer))

    def noise_estimate(self, sum, sq, n, floor=0.01, threshold=0.0, error=None):
        """The noise figure of the image with radiance sums `sum` and square sums `sq` over `n` samples per pixel
        (pathed_hip_noise_estimate_device; the formula is in include/pathed_hip.h): a dict with mean_error, max_error,
        pixels_above (pixels whose error exceeds `threshold`) and invalid_pixels.  `sum` and `sq` are float32 host arrays
        (H, W, 3), uploaded for the call, or device pointers (ints); `error`, if given, receives the per-pixel error: a float32
        host array (H, W) with host sums, a device pointer with device sums."""
        noise = _capi.PathedNoise()
        noise.struct_size = C.sizeof(_capi.PathedNoise)
        if isinstance(sum, np.ndarray) != isinstance(sq, np.ndarray):
            raise TypeError("noise_estimate: `sum` and `sq` must both be host arrays or both be device pointers")
        if not isinstance(sum, np.ndarray):
            code = self._lib.pathed_hip_noise_estimate_device(
                self._handle, C.c_void_p(sum or None), C.c_void_p(sq or None), int(n), float(floor), float(threshold),
                C.c_void_p(error or None), C.byref(noise), None)
            _check(self._lib, code, "pathed_hip_noise_estimate_device")
        else:
            pixels = self.width * self.height
            for array in (sum, sq):
                assert array.dtype == np.float32 and array.size == 3 * pixels
            if error is not None:
                assert error.dtype == np.float32 and error.flags["C_CONTIGUOUS"] and error.size == pixels
            buffers = []
            try:
                buffers.append(self.device_buffer(3 * pixels, sum))
                buffers.append(self.device_buffer(3 * pixels, sq))
                if error is not None:
                    buffers.append(self.device_buffer(pixels))
                code = self._lib.pathed_hip_noise_estimate_device(
                    self._handle, C.c_void_p(buffers[0]), C.c_void_p(buffers[1]), int(n), float(floor), float(threshold),
                    C.c_void_p(buffers[2]) if error is not None else None, C.byref(noise), None)
                _check(self._lib, code, "pathed_hip_noise_estimate_device")
                if error is not None:
                    self.download_device_buffer(buffers[2], error)
            finally:
                for pointer in buffers:
                    self.free_device_buffer(pointer)
        return {"mean_error": noise.mean_error, "max_error": noise.max_error, "pixels_above": int(noise.pixels_above),
                "invalid_pixels": int(noise.invalid_pixels)}

    def device_words(self, count, host=None):
        """`count` uint32 on the scene's device -- a count image or a pixel list -- zeroed or filled from `host`; free with
        free_device_buffer.  (A word is moved as the float of the same bits: the copies are plain memory copies.)"""
        if host is not None:
            host = np.ascontiguousarray(host, dtype=np.uint32).reshape(-1).view(np.float32)
        return self.device_buffer(count, host)

    def download_device_words(self, pointer, out):
        """Copies out.size uint32 from device memory at `pointer` into the uint32 array `out`."""
        assert out.dtype == np.uint32 and out.flags["C_CONTIGUOUS"]
        self.download_device_buffer(pointer, out.view(np.float32))
        return out

    def select_pixels(self, sum_pointer, squares_pointer, count_pointer, list_pointer, floor=0.01, threshold=0.0, error_pointer=0, stream=0):
        """The noise figure with a sample count per pixel, and the pixels still to render (pathed_hip_select_pixels_device):
        device pointers to the two sum images (3 W H floats), the count image (W H uint32), room for W H uint32 at
        `list_pointer` and, optionally, W H floats for the per-pixel error.  The list receives, in ascending order, the pixels
        with error > threshold or fewer than 2 samples.  Returns (n_list, figure) with noise_estimate's figure."""
        noise = _capi.PathedNoise()
        noise.struct_size = C.sizeof(_capi.PathedNoise)
        n_list = C.c_uint32(0)
        code = self._lib.pathed_hip_select_pixels_device(
            self._handle, C.c_void_p(sum_pointer or None), C.c_void_p(squares_pointer or None), C.c_void_p(count_pointer or None),
            float(floor), float(threshold), C.c_void_p(error_pointer or None), C.c_void_p(list_pointer or None), C.byref(n_list),
            C.byref(noise), C.c_void_p(stream))
        _check(self._lib, code, "pathed_hip_select_pixels_device")
        return int(n_list.value), {"mean_error": noise.mean_error, "max_error": noise.max_error, "pixels_above": int(noise.pixels_above),
                                   "invalid_pixels": int(noise.invalid_pixels)}

    def render_pixels(self, seed, spp_begin, spp_count, start_bounce, last_bounce, list_pointer, n_list,
                      sum_pointer, squares_pointer, count_pointer, stream=0):
        """Samples [spp_begin, spp_begin + spp_count) of the `n_list` pixels listed (ascending uint32 pixel indices, device
        memory) and of no other pixel (pathed_hip_render_pixels_device): their sums and square sums continue exactly as
        render_moments_device would continue them, their counts grow by spp_count."""
        code = self._lib.pathed_hip_render_pixels_device(
            self._handle, C.c_uint64(_seed(seed)), spp_begin, spp_count, start_bounce, last_bounce,
            C.c_void_p(list_pointer or None), int(n_list), C.c_void_p(sum_pointer or None), C.c_void_p(squares_pointer or None),
            C.c_void_p(count_pointer or None), C.c_void_p(stream))
        _check(self._lib, code, "pathed_hip_render_pixels_device")

    def render_adaptive(self, seed, spp, start_bounce, last_bounce, target_noise, min_spp=16, floor=0.01, spp_per_launch=1024,
                        on_round=None):
        """Renders until every pixel's own error is at or below `target_noise`, `spp` being the cap -- the schedule of the C++
        host's job key "adaptive" (pathed_amd/host/job.h): min(min_spp, spp) samples of every pixel; then rounds, each of which
        selects the pixels with error > target_noise (select_pixels) and takes them from n to min(2 n, spp) samples
        (render_pixels); the run ends when no pixel is selected or n == spp.  A pixel that is not selected never is again (its
        sums, and so its error, no longer change), so all listed pixels share one count.  Everything stays on the device
        between rounds.  on_round(n, n_list, figure), if given, is called after every selection.
        Returns a dict: sums, squares (H, W, 3) float32, counts (H, W) uint32, rounds, samples_rendered, pixels_at_cap
        (pixels that hold `spp` samples), noise (the figure of the final state) and history [(n, n_list, mean_error)]."""
        seed = _seed(seed)
        if not float(target_noise) > 0.0:
            raise PathedError("target_noise must be a number > 0")
        if int(min_spp) != min_spp or int(min_spp) < 2:
            raise PathedError("min_spp must be an integer >= 2")
        spp, min_spp, spp_per_launch = int(spp), int(min_spp), max(1, int(spp_per_launch))
        pixels = self.width * self.height
        buffers = []
        try:
            sums, squares = self.device_buffer(3 * pixels), None
            buffers.append(sums)
            squares = self.device_buffer(3 * pixels)
            buffers.append(squares)
            n = min(min_spp, spp)
            counts = self.device_words(pixels, np.full(pixels, n, dtype=np.uint32))
            buffers.append(counts)
            pixel_list = self.device_words(pixels)
            buffers.append(pixel_list)
            done = 0
            while done < n:
                count = min(spp_per_launch, n - done)
                self.render_moments_device(seed, done, count, start_bounce, last_bounce, sums, squares)
                done += count
            rounds, rendered, history = 0, n * pixels, []
            while True:
                n_list, figure = self.select_pixels(sums, squares, counts, pixel_list, floor=floor, threshold=target_noise)
                history.append((n, n_list, figure["mean_error"]))
                if on_round is not None:
                    on_round(n, n_list, figure)
                if n_list == 0 or n >= spp:
                    break
                following = min(2 * n, spp)
                done = n
                while done < following:
                    count = min(spp_per_launch, following - done)
                    self.render_pixels(seed, done, count, start_bounce, last_bounce, pixel_list, n_list, sums, squares, counts)
                    done += count
                rendered += (following - n) * n_list
                rounds += 1
                n = following
            out = {"sums": np.zeros((self.height, self.width, 3), dtype=np.float32),
                   "squares": np.zeros((self.height, self.width, 3), dtype=np.float32),
                   "counts": np.zeros((self.height, self.width), dtype=np.uint32)}
            self.download_device_buffer(sums, out["sums"])
            self.download_device_buffer(squares, out["squares"])
            self.download_device_words(counts, out["counts"])
        finally:
            for pointer in buffers:
                self.free_device_buffer(pointer)
        out.update(rounds=rounds, samples_rendered=rendered, pixels_at_cap=int((out["counts"] == spp).sum()), noise=figure, history=history)
        return out

    def trace(self, rays, any_hit=False):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        out = np.zeros(n, dtype=np.int32) if any_hit else np.zeros((n, 4), dtype=np.float32)
        code = self._lib.pathed_hip_trace(
            self._handle, rays.ctypes.data_as(C.POINTER(C.c_float)), n, 1 if any_hit else 0,
            out.ctypes.data_as(C.c_void_p))
        _check(self._lib, code, "pathed_hip_trace")
        return out

    def small_candidates(self, rays):
        """Phase-1 candidate sets of both forms and the set phase 2 accepts (pathed_hip_debug_small_candidates): rays (n, 10) =
        origin, continuation direction, shadow direction, shadow tfar -> (n, 8) uint64, bit p = primitive id p."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 10)
        out = np.zeros((rays.shape[0], 8), dtype=np.uint64)
        code = self._lib.pathed_hip_debug_small_candidates(
            self._handle, rays.ctypes.data_as(C.POINTER(C.c_float)), rays.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint64)))
        _check(self._lib, code, "pathed_hip_debug_small_candidates")
        return out

    def shadow_candidates(self, rays):
        """The shadow ray's pruned phase-1 candidates and the set phase 2 accepts for it (pathed_hip_debug_shadow_candidates):
        rays (n, 10) as small_candidates takes them -> ((n, 2) uint64, bit p = primitive id p; the layout's counts as a dict;
        the never-occluder set as an int, bit p = primitive id p)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 10)
        out = np.zeros((rays.shape[0], 2), dtype=np.uint64)
        layout = (C.c_int32 * 4)()
        never = C.c_uint64(0)
        code = self._lib.pathed_hip_debug_shadow_candidates(
            self._handle, rays.ctypes.data_as(C.POINTER(C.c_float)), rays.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint64)), layout, C.byref(never))
        _check(self._lib, code, "pathed_hip_debug_shadow_candidates")
        counts = {"quads": layout[0], "lone": layout[1], "shadow_quad_pairs": layout[2], "shadow_lone_pairs": layout[3]}
        return out, counts, int(never.value)

    def pass_candidates(self, rays, n_triangles):
        """Both rays' candidates over the fused kernel's pass list -- the item list without exact copies of a lower-numbered
        triangle -- as the timed kernel runs it (pathed_hip_debug_pass_candidates): rays (n, 10) as small_candidates takes them
        -> ((n, 2) uint64 (path ray, shadow ray), bit p = primitive id p; the primitive ids in pass order, (n_triangles,) int32,
        -1 beyond the list; the pass layout's counts as a dict; the never-hit set as an int, bit p = primitive id p)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 10)
        out = np.zeros((rays.shape[0], 2), dtype=np.uint64)
        primitives = np.zeros(n_triangles, dtype=np.int32)
        layout = (C.c_int32 * 5)()
        never = C.c_uint64(0)
        code = self._lib.pathed_hip_debug_pass_candidates(
            self._handle, rays.ctypes.data_as(C.POINTER(C.c_float)), rays.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint64)),
            primitives.ctypes.data_as(C.POINTER(C.c_int32)), n_triangles, layout, C.byref(never))
        _check(self._lib, code, "pathed_hip_debug_pass_candidates")
        counts = {"quads": layout[0], "lone": layout[1], "shadow_quad_pairs": layout[2], "shadow_lone_pairs": layout[3], "triangles": layout[4]}
        return out, primitives, counts, int(never.value)

    def camera_masks(self):
        """The per-pixel candidate masks of the camera rays (pathed_hip_debug_camera_masks; scenes on the fused path kernel):
        (height, width) uint64, bit 63 - k = triangle k of the item order."""
        out = np.zeros((self.height, self.width), dtype=np.uint64)
        code = self._lib.pathed_hip_debug_camera_masks(self._handle, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size)
        _check(self._lib, code, "pathed_hip_debug_camera_masks")
        return out

    def item_order(self, n_triangles):
        """Original primitive id of every item-order triangle (pathed_hip_debug_item_order): (n_triangles,) int32."""
        out = np.zeros(n_triangles, dtype=np.int32)
        code = self._lib.pathed_hip_debug_item_order(self._handle, out.ctypes.data_as(C.POINTER(C.c_int32)), n_triangles)
        _check(self._lib, code, "pathed_hip_debug_item_order")
        return out

    def light_records(self, n_triangles, max_lights):
        """The stored per-triangle and per-light constants beside what the per-vertex functions compute
        (pathed_hip_debug_light_records): (n_triangles, 20) and (the scene's light count, 18) float32."""
        triangles = np.zeros((n_triangles, 20), dtype=np.float32)
        lights = np.zeros((max_lights, 18), dtype=np.float32)
        count = C.c_int(0)
        code = self._lib.pathed_hip_debug_light_records(
            self._handle, triangles.ctypes.data_as(C.POINTER(C.c_float)), n_triangles,
            lights.ctypes.data_as(C.POINTER(C.c_float)), max_lights, C.byref(count))
        _check(self._lib, code, "pathed_hip_debug_light_records")
        return triangles, lights[:count.value]

    def refit(self, positions, normals=None):
        """New vertex positions (and normals) over the same topology (pathed_hip_scene_refit; scenes created with refittable=1).
        Returns the device time of the refit kernels in milliseconds."""
        positions = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        normal_pointer = None
        if normals is not None:
            normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
            assert normals.shape == positions.shape
            normal_pointer = normals.ctypes.data_as(C.POINTER(C.c_float))
        ms = C.c_float(0.0)
        code = self._lib.pathed_hip_scene_refit(self._handle, positions.ctypes.data_as(C.POINTER(C.c_float)), normal_pointer,
                                                positions.shape[0], C.byref(ms))
        _check(self._lib, code, "pathed_hip_scene_refit")
        return float(ms.value)

    def set_instance_transforms(self, transforms):
        """New transforms for all placements of an instanced scene (pathed_hip_scene_set_instance_transforms): the records are
        restated and the top tree refitted on the device; prototypes, instance count and primitive ids stay.  `transforms` is
        an (n, 12) or (n, 3, 4) float32 numpy array (row-major 3 x 4 each, instance order), or a contiguous float32 torch
        tensor of that shape on the scene's device, read in place (the _device entry).  Host data keeps `self.instance_set` in
        step, so that flatten_instances still describes the scene; after device data it describes the placements of the last
        host call.  Returns the device time of the kernels in milliseconds."""
        ms = C.c_float(0.0)
        if hasattr(transforms, "data_ptr"):
            import torch
            if not (transforms.is_cuda and transforms.device.index == self.device):
                raise ValueError("the transforms tensor must live on the scene's device (cuda:%d)" % self.device)
            if transforms.dtype != torch.float32 or not transforms.is_contiguous() or transforms.numel() % 12 != 0:
                raise ValueError("the transforms tensor must be contiguous float32, 12 values per instance")
            # the tensor may keep some storage address even when it is empty; the count alone decides what is read
            pointer = C.c_void_p(transforms.data_ptr() or 0)
            code = self._lib.pathed_hip_scene_set_instance_transforms_device(self._handle, pointer, transforms.numel() // 12, C.byref(ms))
            _check(self._lib, code, "pathed_hip_scene_set_instance_transforms_device")
            return float(ms.value)
        transforms = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 12)
        padded = transforms if len(transforms) else np.zeros((1, 12), dtype=np.float32)   # (an empty array has no address to pass)
        code = self._lib.pathed_hip_scene_set_instance_transforms(self._handle, padded.ctypes.data_as(C.POINTER(C.c_float)), len(transforms), C.byref(ms))
        _check(self._lib, code, "pathed_hip_scene_set_instance_transforms")
        if getattr(self, "instance_set", None) is not None:
            self.instance_set.set_transforms(transforms)
        return float(ms.value)

    def set_instance_motion(self, transforms_close, shutter=(0.0, 1.0)):
        """The placements at shutter time 1 (pathed_hip_scene_set_instance_motion); the scene's current transforms are the
        placements at time 0.  Every sample then sees each moving placement at its own time, `instances.sample_time` of
        (seed, pixel, sample), under `instances.interpolate_transforms`; a placement whose two transforms are bit-equal does not
        move.  `transforms_close` as set_instance_transforms takes them (numpy, or a torch tensor on the scene's device);
        `shutter` = (open, close) with 0 <= open <= close <= 1.  Returns the device time of the kernels in milliseconds."""
        ms = C.c_float(0.0)
        shutter_open, shutter_close = C.c_float(float(shutter[0])), C.c_float(float(shutter[1]))
        if hasattr(transforms_close, "data_ptr"):
            import torch
            if not (transforms_close.is_cuda and transforms_close.device.index == self.device):
                raise ValueError("the transforms tensor must live on the scene's device (cuda:%d)" % self.device)
            if transforms_close.dtype != torch.float32 or not transforms_close.is_contiguous() or transforms_close.numel() % 12 != 0:
                raise ValueError("the transforms tensor must be contiguous float32, 12 values per instance")
            if transforms_close.numel() == 0:
                raise ValueError("an empty tensor names no motion: clear_instance_motion() removes one")
            code = self._lib.pathed_hip_scene_set_instance_motion_device(self._handle, C.c_void_p(transforms_close.data_ptr()), transforms_close.numel() // 12,
                                                                        shutter_open, shutter_close, C.byref(ms))
            _check(self._lib, code, "pathed_hip_scene_set_instance_motion_device")
            return float(ms.value)
        transforms_close = np.ascontiguousarray(transforms_close, dtype=np.float32).reshape(-1, 12)
        padded = transforms_close if len(transforms_close) else np.zeros((1, 12), dtype=np.float32)   # (an empty array has no address to pass)
        code = self._lib.pathed_hip_scene_set_instance_motion(self._handle, padded.ctypes.data_as(C.POINTER(C.c_float)), len(transforms_close),
                                                             shutter_open, shutter_close, C.byref(ms))
        _check(self._lib, code, "pathed_hip_scene_set_instance_motion")
        return float(ms.value)

    def clear_instance_motion(self):
        """Removes the motion (pathed_hip_scene_set_instance_motion with no transforms): the static boxes are restored and
        renders are the static scene's bits again.  Returns the device time of the refit in milliseconds."""
        ms = C.c_float(0.0)
        code = self._lib.pathed_hip_scene_set_instance_motion(self._handle, None, 0, C.c_float(0.0), C.c_float(1.0), C.byref(ms))
        _check(self._lib, code, "pathed_hip_scene_set_instance_motion")
        return float(ms.value)

    def trace_timed(self, rays, times, any_hit=False):
        """`trace` with one shutter time per ray, on a scene with motion (pathed_hip_trace_timed)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        times = np.ascontiguousarray(times, dtype=np.float32).reshape(-1)
        n = rays.shape[0]
        if len(times) != n:
            raise ValueError("%d times for %d rays" % (len(times), n))
        out = np.zeros(n, dtype=np.int32) if any_hit else np.zeros((n, 4), dtype=np.float32)
        code = self._lib.pathed_hip_trace_timed(
            self._handle, rays.ctypes.data_as(C.POINTER(C.c_float)), times.ctypes.data_as(C.POINTER(C.c_float)), n, 1 if any_hit else 0,
            out.ctypes.data_as(C.c_void_p))
        _check(self._lib, code, "pathed_hip_trace_timed")
        return out

    def rebuild_top(self, builder="ploc"):
        """A new top tree over the world triangles and the placements' current world boxes, built on the device
        (pathed_hip_scene_rebuild_top): what follows set_instance_transforms when the placements were scattered far, since a
        refit keeps the tree's shape.  `builder` is "lbvh", "ploc" or the PATHED_BVH_* constant (1, 2); the host builder ("sah")
        is refused by the library: it needs the scene created again.  Returns the device time in milliseconds."""
        kind = self.BVH_BUILDERS[builder] if isinstance(builder, str) else int(builder)
        ms = C.c_float(0.0)
        _check(self._lib, self._lib.pathed_hip_scene_rebuild_top(self._handle, kind, C.byref(ms)), "pathed_hip_scene_rebuild_top")
        return float(ms.value)

    def instance_records(self):
        """The placements' records as the device holds them (pathed_hip_debug_instance_records): (transforms (n, 12) float32,
        inverses (n, 12) float32, ids (n, 4) int32: virtual id base, prototype, its root node, its first shading record)."""
        count = int(self.instance_set.desc.n_instances) if getattr(self, "instance_set", None) is not None else 0
        records = np.zeros((max(1, count), 28), dtype=np.float32)
        code = self._lib.pathed_hip_debug_instance_records(self._handle, records.ctypes.data_as(C.POINTER(C.c_float)), count)
        _check(self._lib, code, "pathed_hip_debug_instance_records")
        records = records[:count]
        return records[:, 0:12].copy(), records[:, 12:24].copy(), records[:, 24:28].copy().view(np.int32)

    def set_samples_per_unit(self, samples):
        """Summation granularity (see include/pathed_hip.h); 1 = the reference's exact order."""
        _check(self._lib, self._lib.pathed_hip_set_samples_per_unit(self._handle, int(samples)),
               "pathed_hip_set_samples_per_unit")

    def set_camera(self, camera):
        """Another view of the same scene (pathed_hip_scene_set_camera): `camera` is a _capi.PathedCamera of the scene's resolution."""
        _check(self._lib, self._lib.pathed_hip_scene_set_camera(self._handle, C.byref(camera)), "pathed_hip_scene_set_camera")

    def set_grid_medium(self, medium_index, grid=None, *, data=None, bounds=None, albedo=1.0, scale=1.0, world_to_model=None, model_to_world=None):
        """Turn medium slot `medium_index` into a voxel-grid medium (pathed_hip_scene_set_grid_medium), or replace its grid.
        Either `grid`, a _capi.PathedGridMedium (LoadedScene.grids carries those of a scene file), or `data`, a float array of
        shape (cells_z, cells_y, cells_x), with `bounds` = (min x, y, z, max x, y, z) and the two row-major 4x4 matrices
        (identity when absent; one given, the other is its numpy inverse)."""
        if grid is None:
            data = np.ascontiguousarray(data, dtype=np.float32)
            assert data.ndim == 3 and bounds is not None and len(bounds) == 6
            if world_to_model is None and model_to_world is None:
                world_to_model = model_to_world = np.eye(4)
            elif model_to_world is None:
                model_to_world = np.linalg.inv(np.asarray(world_to_model, dtype=np.float64))
            elif world_to_model is None:
                world_to_model = np.linalg.inv(np.asarray(model_to_world, dtype=np.float64))
            grid = _capi.PathedGridMedium()
            grid.cells_z, grid.cells_y, grid.cells_x = data.shape
            grid.bounds[:] = [float(value) for value in bounds]
            grid.data = data.ctypes.data_as(C.POINTER(C.c_float))
            grid.albedo, grid.scale = float(albedo), float(scale)
            grid.world_to_model[:] = [float(value) for value in np.asarray(world_to_model, dtype=np.float32).reshape(16)]
            grid.model_to_world[:] = [float(value) for value in np.asarray(model_to_world, dtype=np.float32).reshape(16)]
        grid.struct_size = C.sizeof(_capi.PathedGridMedium)
        _check(self._lib, self._lib.pathed_hip_scene_set_grid_medium(self._handle, int(medium_index), C.byref(grid)), "pathed_hip_scene_set_grid_medium")

    def grid_queries(self, medium_index, a, b, target):
        """GridMedium::transmittance(a, b) and findTransmittance(a, b, target) of the grid in slot `medium_index` for n world-space
        segments (pathed_hip_grid_queries): (transmittance, distance), float32 (n,); distance is -1 where the result is invalid."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
        target = np.ascontiguousarray(target, dtype=np.float32).reshape(-1)
        assert a.shape == b.shape and target.shape[0] == a.shape[0]
        transmittance = np.zeros(a.shape[0], dtype=np.float32)
        distance = np.zeros(a.shape[0], dtype=np.float32)
        pointer = lambda array: array.ctypes.data_as(C.POINTER(C.c_float))
        _check(self._lib, self._lib.pathed_hip_grid_queries(self._handle, int(medium_index), a.shape[0], pointer(a), pointer(b), pointer(target),
                                                            pointer(transmittance), pointer(distance)), "pathed_hip_grid_queries")
        return transmittance, distance

    def shading_queries(self, function, traits, records):
        """One shading function per record on the device (pathed_hip_debug_shading_queries): `function` a key of
        _capi.SHADING_QUERIES, `traits` one of _capi.SHADING_TRAITS, records (n, floats in) in the layouts of
        tests/golden/README.md -> (n, floats out) float32."""
        code, n_in, n_out = _capi.SHADING_QUERIES[function]
        records = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, n_in)
        out = np.zeros((records.shape[0], n_out), dtype=np.float32)
        pointer = lambda array: array.ctypes.data_as(C.POINTER(C.c_float))
        _check(self._lib, self._lib.pathed_hip_debug_shading_queries(self._handle, code, _capi.SHADING_TRAITS[traits], records.shape[0],
                                                                     pointer(records), pointer(out)), "pathed_hip_debug_shading_queries")
        return out

    def phase_samples(self, u):
        """The device's phase-function sample (pathed_hip_debug_phase_samples) on scripted numbers: u (n, 2) in [0, 1] ->
        directions (n, 3) float32, (r cos phi, z, r sin phi) with z = 2 u[0] - 1 and phi = 2 pi u[1]."""
        u = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 2)
        out = np.zeros((u.shape[0], 3), dtype=np.float32)
        pointer = lambda array: array.ctypes.data_as(C.POINTER(C.c_float))
        _check(self._lib, self._lib.pathed_hip_debug_phase_samples(self._handle, u.shape[0], pointer(u), pointer(out)), "pathed_hip_debug_phase_samples")
        return out

    def set_medium_phase(self, medium_index, g, type_="henyey-greenstein"):
        """The phase function of medium slot `medium_index` (pathed_hip_scene_set_medium_phase): "henyey-greenstein" with mean
        cosine g (|g| <= 0.99; g > 0 scatters forward) or "isotropic".  Calling it again replaces the entry."""
        phase = _capi.PathedPhaseFunction()
        phase.struct_size = C.sizeof(_capi.PathedPhaseFunction)
        phase.type = {"isotropic": _capi.PHASE_ISOTROPIC, "henyey-greenstein": _capi.PHASE_HENYEY_GREENSTEIN}[type_] if isinstance(type_, str) else int(type_)
        phase.g = float(g)
        _check(self._lib, self._lib.pathed_hip_scene_set_medium_phase(self._handle, int(medium_index), C.byref(phase)), "pathed_hip_scene_set_medium_phase")

    def phase_hg(self, records):
        """The device's Henyey-Greenstein sample and value (pathed_hip_debug_phase_hg): records (n, 9) = (g, w(3), u1, u2, wi(3))
        -> (n, 4) float32: the direction sampled about w, then p(w, wi)."""
        records = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 9)
        out = np.zeros((records.shape[0], 4), dtype=np.float32)
        pointer = lambda array: array.ctypes.data_as(C.POINTER(C.c_float))
        _check(self._lib, self._lib.pathed_hip_debug_phase_hg(self._handle, records.shape[0], pointer(records), pointer(out)), "pathed_hip_debug_phase_hg")
        return out

    def set_integrator(self, name):
        """"PathTracer" (default), "VolumePathTracer", "BasicVolumeIntegrator" or "AlbedoIntegrator" (reference src/job.cpp:65-97)."""
        code = {"PathTracer": _capi.INTEGRATOR_PATH_TRACER, "DataParallelIntegrator": _capi.INTEGRATOR_PATH_TRACER,
                "VolumePathTracer": _capi.INTEGRATOR_VOLUME_PATH_TRACER, "AlbedoIntegrator": _capi.INTEGRATOR_ALBEDO,
                "BasicVolumeIntegrator": _capi.INTEGRATOR_BASIC_VOLUME}[name]
        _check(self._lib, self._lib.pathed_hip_set_integrator(self._handle, code), "pathed_hip_set_integrator")

    def set_stats_mode(self, count=False, time_kernels=False, time_sampled=False):
        """time_kernels: HIP events around every launch; time_sampled: around every 8th (cheaper, same averages)."""
        mode = (1 if count else 0) | (2 if time_kernels else 0) | (4 if time_sampled else 0)
        _check(self._lib, self._lib.pathed_hip_set_stats_mode(self._handle, mode), "pathed_hip_set_stats_mode")

    def reset_stats(self):
        _check(self._lib, self._lib.pathed_hip_reset_stats(self._handle), "pathed_hip_reset_stats")

    def stats(self):
        stats = _capi.PathedStats()
        _check(self._lib, self._lib.pathed_hip_get_stats(self._handle, C.byref(stats)), "pathed_hip_get_stats")
        return {name: getattr(stats, name) for name, _ in _capi.PathedStats._fields_}

    def export_bvh(self):
        n_nodes, n_tris = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib, self._lib.pathed_hip_scene_export_bvh(self._handle, None, C.byref(n_nodes), None, C.byref(n_tris)),
               "pathed_hip_scene_export_bvh")
        nodes = np.zeros((n_nodes.value, 32), dtype=np.float32)
        tris = np.zeros((n_tris.value, 12), dtype=np.float32)
        _check(self._lib, self._lib.pathed_hip_scene_export_bvh(
            self._handle, nodes.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n_nodes),
            tris.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n_tris)), "pathed_hip_scene_export_bvh")
        return nodes, tris

    def export_compressed_nodes(self):
        """(n, 16) or (n, 32) uint32 words of the compressed nodes (include/pathed_hip.h), n = 0 when the scene carries none"""
        n_nodes, words = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib, self._lib.pathed_hip_scene_export_compressed_nodes(self._handle, None, C.byref(n_nodes), C.byref(words)),
               "pathed_hip_scene_export_compressed_nodes")
        nodes = np.zeros((n_nodes.value, words.value or 16), dtype=np.uint32)
        if n_nodes.value:
            _check(self._lib, self._lib.pathed_hip_scene_export_compressed_nodes(
                self._handle, nodes.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n_nodes), C.byref(words)), "pathed_hip_scene_export_compressed_nodes")
        return nodes


class BounceController:
    """reference src/bounce_controller.cpp:5-25"""

    def __init__(self, start_bounce, last_bounce):
        assert start_bounce >= 0
        assert last_bounce == -1 or start_bounce <= last_bounce
        self.start_bounce = start_bounce
        self.last_bounce = last_bounce

    def check_done(self, bounce):
        if self.last_bounce == -1:
            return False
        return bounce > self.last_bounce

    def check_counts(self, bounce):
        if self.start_bounce > bounce:
            return False
        return not self.check_done(bounce)


class PathTracer:
    """GPU stand-in for the reference's PathTracer integrator.

    `run(image, scene, callback, quit)` keeps the reference's contract: `image` receives
    sum/(i+1) after every batch, checkpoints are reported at power-of-two sample counts.
    Instead of one wave per call it renders `spp_per_launch` samples per launch (the
    reference's PDFIntegrator also overrides run()).
    """

    def __init__(self, bounce_controller, spp=1, seed=1, spp_per_launch=1024, target_noise=None, min_spp=16, noise_floor=0.01, adaptive=False):
        self.bounce_controller = bounce_controller
        self.spp = spp
        self.seed = _seed(seed)
        if int(spp_per_launch) < 1:
            raise PathedError("spp_per_launch must be >= 1")
        self.spp_per_launch = int(spp_per_launch)
        # noise-targeted stopping: the twin of the C++ host's job keys (pathed_amd/host/job.h)
        if target_noise is not None and not float(target_noise) > 0.0:
            raise PathedError("target_noise must be a number > 0")
        if int(min_spp) != min_spp or int(min_spp) < 2:
            raise PathedError("min_spp must be an integer >= 2")
        if not float(noise_floor) > 0.0:
            raise PathedError("noise_floor must be a number > 0")
        self.target_noise = None if target_noise is None else float(target_noise)
        self.min_spp = int(min_spp)
        self.noise_floor = float(noise_floor)
        self.noise_history = []      # (spp, mean_error) at every checkpoint the figure was estimated at
        self.stopped_on_noise = False
        # adaptive sampling (job key "adaptive"): the target holds per pixel, and only the pixels above it are rendered on
        if adaptive and target_noise is None:
            raise PathedError("adaptive needs target_noise")
        self.adaptive = bool(adaptive)
        self.sample_counts = None    # (H, W) uint32 after an adaptive run
        self.adaptive_result = None  # ... and HipScene.render_adaptive's dict

    def _run_adaptive(self, image, scene, callback):
        """run() with adaptive=True: HipScene.render_adaptive; the image is sum / count per pixel.  The callback is called after
        every selection with the sample count of the pixels still active (noise_history gets the image's mean error there)."""
        self.noise_history = []

        def on_round(n, n_list, figure):
            self.noise_history.append((n, figure["mean_error"]))
            if callback is not None:
                callback(n, (n & (n - 1)) == 0)

        result = scene.render_adaptive(self.seed, self.spp, self.bounce_controller.start_bounce, self.bounce_controller.last_bounce,
                                       self.target_noise, min_spp=self.min_spp, floor=self.noise_floor,
                                       spp_per_launch=self.spp_per_launch, on_round=on_round)
        self.adaptive_result = result
        self.sample_counts = result["counts"]
        self.stopped_on_noise = result["history"][-1][1] == 0
        np.divide(result["sums"], result["counts"][..., None].astype(np.float32), out=image)
        return image

    def _run_to_noise_target(self, image, scene, callback, quit_flag):
        """run() with a target: the sums and their squares stay on the device and continue there (render_moments_device), the
        figure is estimated at the power-of-two checkpoints from min_spp on and at the end, and the run stops at the first one
        at or below the target -- batch for batch what the C++ host does (pathed_amd/host/integrator.cpp)."""
        floats = 3 * scene.width * scene.height
        sums = np.zeros((scene.height, scene.width, 3), dtype=np.float32)
        self.noise_history = []
        self.stopped_on_noise = False
        buffers = []
        try:
            buffers.append(scene.device_buffer(floats))
            buffers.append(scene.device_buffer(floats))
            done = 0
            while done < self.spp:
                next_power = 1
                while next_power <= done:
                    next_power *= 2
                count = min(self.spp_per_launch, self.spp - done, next_power - done)
                scene.render_moments_device(self.seed, done, count, self.bounce_controller.start_bounce,
                                            self.bounce_controller.last_bounce, buffers[0], buffers[1])
                done += count
                scene.download_device_buffer(buffers[0], sums)
                np.divide(sums, np.float32(done), out=image)
                checkpoint = (done & (done - 1)) == 0
                if callback is not None:
                    callback(done, checkpoint)
                if (checkpoint or done == self.spp) and done >= self.min_spp:
                    figure = scene.noise_estimate(buffers[0], buffers[1], done, floor=self.noise_floor, threshold=self.target_noise)
                    self.noise_history.append((done, figure["mean_error"]))
                    if figure["mean_error"] <= self.target_noise and done < self.spp:
                        self.stopped_on_noise = True
                        break
                if quit_flag is not None and quit_flag():
                    return
        finally:
            for pointer in buffers:
                scene.free_device_buffer(pointer)
        return image

    def run(self, image, scene, callback=None, quit_flag=None):
        """image: float32 (H, W, 3) array that receives the running mean; scene: HipScene.  With target_noise the run may end
        before `spp` (stopped_on_noise, noise_history)."""
        if self.adaptive:
            return self._run_adaptive(image, scene, callback)
        if self.target_noise is not None:
            return self._run_to_noise_target(image, scene, callback, quit_flag)
        radiance_lookup = np.zeros((scene.height, scene.width, 3), dtype=np.float32)
        done = 0
        while done < self.spp:
            # stop at the next power of two so checkpoints land exactly where the reference writes them
            next_power = 1
            while next_power <= done:
                next_power *= 2
            count = min(self.spp_per_launch, self.spp - done, next_power - done)
            scene.render(self.seed, done, count, self.bounce_controller.start_bounce,
                         self.bounce_controller.last_bounce, radiance_lookup)
            done += count
            np.divide(radiance_lookup, np.float32(done), out=image)
            if callback is not None:
                callback(done, (done & (done - 1)) == 0)
            if quit_flag is not None and quit_flag():
                return
        return image


INTEGRATOR_NAMES = ("PathTracer", "DataParallelIntegrator", "VolumePathTracer", "AlbedoIntegrator", "BasicVolumeIntegrator")
FEATURE_NAMES = ("albedo", "normal", "depth")


def features_from_job(job):
    """The job key "features": a list drawn from FEATURE_NAMES, absent = none.  An unknown name is an error that names it."""
    wanted = job.get("features", [])
    if not isinstance(wanted, (list, tuple)):
        raise PathedError("job: \"features\" must be a list of names out of %s" % ", ".join(FEATURE_NAMES))
    for name in wanted:
        if name not in FEATURE_NAMES:
            raise PathedError("job: unknown feature \"%s\" (known: %s)" % (name, ", ".join(FEATURE_NAMES)))
    return [name for name in FEATURE_NAMES if name in wanted]


def seed_from_job(job):
    """The job key "seed" (default 1): any integer in [0, 2^64), read exactly as written.  A negative, fractional or over-range
    value, one written with an exponent (json reads it as a float) and anything that is not a number are refused by name, in
    the C++ host's words (pathed_amd/host/job.cpp)."""
    value = job.get("seed", 1)
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value < 1 << 64:
        raise PathedError("job: \"seed\" must be %s, written in plain digits" % SEED_RANGE)
    return value


def noise_from_job(job):
    """The job keys "target_noise" (a number > 0, absent = none), "min_spp" (an integer >= 2, default 16), "noise_floor"
    (a number > 0, default 0.01) and "stderr_image" (a bool, implied by a target): (target_noise or None, min_spp, floor,
    write_stderr).  A bad value is an error that names its key, and so is "resume" beside either key: the state file
    holds no squares."""
    def number(value):
        return isinstance(value, (int, float)) and not isinstance(value, bool)
    target = job.get("target_noise")
    if target is not None and not (number(target) and 0.0 < target < 1e30):
        raise PathedError("job: \"target_noise\" must be a number > 0")
    min_spp = job.get("min_spp", 16)
    if not (number(min_spp) and int(min_spp) == min_spp and 2 <= min_spp <= 1e9):
        raise PathedError("job: \"min_spp\" must be an integer >= 2")
    floor = job.get("noise_floor", 0.01)
    if not (number(floor) and 0.0 < floor < 1e30):
        raise PathedError("job: \"noise_floor\" must be a number > 0")
    write_stderr = job.get("stderr_image", False)
    if not isinstance(write_stderr, bool):
        raise PathedError("job: \"stderr_image\" must be true or false")
    write_stderr = write_stderr or target is not None
    if write_stderr and job.get("resume", False):
        raise PathedError("job: \"resume\" does not go with \"%s\": the state file holds no squares"
                          % ("target_noise" if target is not None else "stderr_image"))
    return (None if target is None else float(target)), int(min_spp), float(floor), write_stderr


def adaptive_from_job(job):
    """The job key "adaptive" (a bool, default false): render on only the pixels whose own error is above "target_noise"
    (pathed_amd/host/job.h has the schedule).  It needs "target_noise" and one GPU, and goes neither with "resume" nor with the
    AlbedoIntegrator; every refusal names the key."""
    adaptive = job.get("adaptive", False)
    if not isinstance(adaptive, bool):
        raise PathedError("job: \"adaptive\" must be true or false")
    if not adaptive:
        return False
    if job.get("target_noise") is None:
        raise PathedError("job: \"adaptive\" needs \"target_noise\": the pixels above it are the ones rendered on")
    if job.get("resume", False):
        raise PathedError("job: \"adaptive\" does not go with \"resume\": the state file holds neither squares nor counts")
    gpus = job.get("gpus", 1)
    if (len(gpus) if isinstance(gpus, (list, tuple)) else gpus) != 1:
        raise PathedError("job: \"adaptive\" renders on one GPU: \"gpus\" must be 1 (a pixel list is not sharded)")
    if job.get("integrator") == "AlbedoIntegrator":
        raise PathedError("job: \"adaptive\" does not go with the AlbedoIntegrator, which keeps no second moments")
    return True


def integrator_from_job(job, **kwargs):
    """reference Job::integrator(), src/job.cpp:65-97 — only the hot-path integrator exists here."""
    name = job["integrator"]
    if name in INTEGRATOR_NAMES:
        # the caller selects the arithmetic on the scene: HipScene.set_integrator(name)
        return PathTracer(BounceController(job["startBounce"], job["lastBounce"]),
                          spp=job["spp"] if job["spp"] > 0 else 9999999, **kwargs)
    raise PathedError("Unimplemented")
