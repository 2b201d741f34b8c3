/*
 * pathed_hip.h — C ABI of the MI355X path-tracing integrator (libpathed_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of chellmuth/pathed: the per-pixel
 * radiance loop  Integrator::run -> SampleIntegrator::sampleImage/samplePixel ->
 * PathTracer::L / direct  (reference src/integrator.cpp:19-106,
 * src/sample_integrator.cpp:10-113, src/path_tracer.cpp:19-216) together with the
 * ray queries it makes through Scene (reference src/scene.cpp:91-223, 355-381,
 * 446-502), which the reference forwards to Embree (rtcIntersect1 / rtcOccluded1).
 *
 * The reference has no FFI: its plug-in surface is the C++ virtual class
 * `Integrator` (reference include/integrator.h:16-55) chosen by the "integrator"
 * string of job.json (reference src/job.cpp:65-97).  A GPU integrator subclasses
 * `Integrator`, overrides run(), and calls the functions below.  The binding a
 * reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every call returns 0 on success
 *     or a negative PATHED_E_* code, message via pathed_hip_last_error()
 *     (reference error behaviour: throw "Unimplemented" / std::runtime_error /
 *     exit(1), src/job.cpp:96, src/scene_parser.cpp:665, src/glass.cpp:69-72).
 *   - caller owns every array in PathedSceneDesc; scene_create copies what it needs.
 *   - a PathedScene is used by one host thread at a time; render calls block.
 *   - all arithmetic is IEEE fp32; indices are int32/uint32.
 */
#ifndef PATHED_HIP_H
#define PATHED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PATHED_ABI_VERSION 4   /* 2: image-texture albedo (PathedTexture, PathedMaterial.texture)
                                * 3: participating media (PathedMedium, PathedGeom.medium, PATHED_MAT_PASSTHROUGH)
                                * 4: the process-global pathed_hip_set_bvh_builder is gone (PathedSceneOptions.bvh_builder);
                                *    PathedSceneOptions.build_threads; pathed_hip_comm_* (RCCL reduce of the radiance sums) */
/* Additions that leave PathedSceneDesc unchanged (no version bump): PathedSceneOptions /
 * pathed_hip_scene_create_ex (per-scene device and tuning), pathed_hip_measure_valu,
 * pathed_hip_accum_add / pathed_hip_accum_copy_peer (multi-GPU fan-in of the radiance sums),
 * PathedFeatureBuffers / pathed_hip_render_features[_device] (first-hit feature images), PATHED_INTEGRATOR_ALBEDO,
 * pathed_hip_render_moments[_device] / PathedNoise / pathed_hip_noise_estimate_device (per-pixel second moments and the noise figure),
 * pathed_hip_select_pixels_device / pathed_hip_render_pixels_device (adaptive sampling over pixel lists),
 * PathedInstanceDesc / pathed_hip_scene_create_instanced (instanced geometry). */

/* error codes */
#define PATHED_OK            0
#define PATHED_E_INVALID    -1   /* bad argument / malformed scene description   */
#define PATHED_E_DEVICE     -2   /* HIP runtime error (message has the HIP text)  */
#define PATHED_E_NO_DEVICE  -3   /* no usable gfx950 device                        */
#define PATHED_E_UNSUPPORTED -4  /* feature outside the hot-path scope             */
#define PATHED_E_NOMEM      -5

/* material kinds — reference Material subclasses on the hot path
 * (src/lambertian.cpp, src/oren_nayar.cpp, src/microfacet.cpp + src/beckmann.cpp,
 *  src/plastic.cpp, src/glass.cpp, src/mirror.cpp) */
#define PATHED_MAT_LAMBERTIAN 0
#define PATHED_MAT_OREN_NAYAR 1
#define PATHED_MAT_MICROFACET 2
#define PATHED_MAT_PLASTIC    3
#define PATHED_MAT_GLASS      4
#define PATHED_MAT_MIRROR     5
#define PATHED_MAT_PASSTHROUGH 6 /* reference src/passthrough.cpp: the boundary of a participating medium ("container") */

/* Lambertian albedo source (reference include/albedo.h, src/checkerboard.cpp:9-20) */
#define PATHED_ALBEDO_CONSTANT     0
#define PATHED_ALBEDO_CHECKERBOARD 1
#define PATHED_ALBEDO_TEXTURE      2   /* reference src/texture.cpp:33-49 */

/* microfacet distribution (reference src/scene_parser.cpp:669-683) */
#define PATHED_DIST_BECKMANN 0
#define PATHED_DIST_GGX      1   /* reference src/ggx.cpp */

/* geometry kinds in model order (reference src/scene_parser.cpp:251-291) */
#define PATHED_GEOM_MESH   0
#define PATHED_GEOM_SPHERE 1

/* Camera — reference Camera ctor arguments (src/camera.cpp:13-30), as parsed by
 * src/scene_parser.cpp:146-158.  vertical_fov is already in radians. */
typedef struct PathedCamera {
    float origin[3];
    float target[3];
    float up[3];
    float vertical_fov;      /* radians */
    int32_t width;           /* job.json "width"  (reference include/job.h:24) */
    int32_t height;          /* job.json "height" (reference include/job.h:25) */
    int32_t flip_handedness; /* scene "sensor.flipHandedness"                  */
} PathedCamera;

/* One BSDF.  Only the fields of `type` are read.
 * emit != 0 makes every surface with this material an area light
 * (reference src/scene_parser.cpp:173-183). */
typedef struct PathedMaterial {
    int32_t type;            /* PATHED_MAT_*                                   */
    int32_t albedo_type;     /* PATHED_ALBEDO_* (Lambertian / Plastic diffuse) */
    float diffuse[3];        /* Lambertian, OrenNayar, Plastic                 */
    float emit[3];           /* Material::emit()                               */
    float checker_on[3];     /* Checkerboard onColor                           */
    float checker_off[3];    /* Checkerboard offColor                          */
    float checker_res[2];    /* Checkerboard resolution (u, v)                 */
    float sigma;             /* OrenNayar sigma (A, B derived as oren_nayar.cpp:11-18) */
    float alpha;             /* Beckmann alpha                                 */
    float ior;               /* Glass ior (reference default 1.4, glass.cpp:16-18) */
    int32_t distribution;    /* PATHED_DIST_*                                  */
    int32_t texture;         /* PATHED_ALBEDO_TEXTURE: index into PathedSceneDesc.textures */
} PathedMaterial;

/* Image texture — reference Texture (src/texture.cpp): what stbi_load(path, .., 3) returns,
 * 8-bit RGB, row 0 = first row of the file.  The lookup wraps uv, flips v, rounds to the
 * nearest texel and applies powf(x / 255, 2.2) (texture.cpp:33-49). */
typedef struct PathedTexture {
    int32_t width;           /* 1 .. 65535                                     */
    int32_t height;
    const uint8_t *rgb;      /* 3*width*height                                 */
} PathedTexture;

/* Sphere — reference Sphere (src/sphere.cpp).  The reference intersects the
 * TRANSFORMED centre (sphere.cpp:30-35) but samples the UNTRANSFORMED m_center
 * (sphere.cpp:77-128); both are carried so that quirk is reproducible. */
typedef struct PathedSphere {
    float center_world[3];
    float radius;
    float center_sample[3];
    int32_t material;
} PathedSphere;

/* One entry per model of the scene JSON, in file order (= Embree geomID order,
 * reference src/rtc_manager.cpp:12-27).  Light order follows it
 * (reference src/scene_parser.cpp:173-183). */
typedef struct PathedGeom {
    int32_t type;   /* PATHED_GEOM_*                                            */
    int32_t first;  /* MESH: first triangle index; SPHERE: index into spheres  */
    int32_t count;  /* MESH: triangle count;       SPHERE: 1                   */
    int32_t medium; /* the model's "internal_medium" (reference src/scene_parser.cpp:324-337, Surface::getInternalMedium):
                       index into PathedSceneDesc.media, -1 = none               */
} PathedGeom;

/* Homogeneous participating medium — reference HomogeneousMedium (src/homogeneous_medium.cpp; scene JSON "media",
 * src/scene_parser.cpp:221-226).  The reference's transmittance uses all three channels of sigma_t, its distance
 * sampling the red one (it asserts the three are equal). */
typedef struct PathedMedium {
    float sigma_t[3];
    float sigma_s[3];
} PathedMedium;

/* Environment light — reference EnvironmentLight (src/environment_light.cpp).
 * rgba is the float RGBA image LoadEXR returns (row 0 = theta 0), map_to_world /
 * world_to_map are the 4x4 row-major matrices parseTransform builds
 * (src/scene_parser.cpp:690-793). */
typedef struct PathedEnvLight {
    int32_t width;
    int32_t height;
    const float *rgba;        /* 4*width*height                                 */
    float scale;
    float map_to_world[16];
    float world_to_map[16];
} PathedEnvLight;

/* Flat scene description: what the reference hands Embree
 * (src/geometry_parser.cpp:12-96: vertex / index / uv / normal buffers per mesh)
 * plus its material, light and camera objects. */
typedef struct PathedSceneDesc {
    uint32_t abi_version;     /* PATHED_ABI_VERSION                             */

    PathedCamera camera;

    /* triangle soup, all meshes concatenated in geom order */
    uint32_t n_vertices;
    const float *positions;   /* 3*n_vertices, world space                      */
    const float *normals;     /* 3*n_vertices, zero vector = "no normal"        */
    const float *uvs;         /* 2*n_vertices                                   */
    uint32_t n_triangles;
    const uint32_t *indices;  /* 3*n_triangles, into the vertex arrays          */
    const int32_t *tri_material; /* n_triangles, index into materials           */

    uint32_t n_spheres;
    const PathedSphere *spheres;

    uint32_t n_geoms;
    const PathedGeom *geoms;

    uint32_t n_materials;
    const PathedMaterial *materials;

    const PathedEnvLight *env; /* NULL = no environment light                   */

    uint32_t n_textures;
    const PathedTexture *textures;

    uint32_t n_media;
    const PathedMedium *media;
} PathedSceneDesc;

typedef struct PathedScene PathedScene;   /* opaque; owns all device memory     */

/* Counters filled by the instrumented ("stats") variants of the kernels and by the
 * timed renders; see DESIGN.md "Algorithmic bytes". */
typedef struct PathedStats {
    uint64_t camera_samples;       /* paths started                              */
    uint64_t closest_rays;         /* closest-hit queries traced                 */
    uint64_t shadow_rays;          /* any-hit queries traced                     */
    uint64_t nodes_visited;        /* child boxes tested (32 B each: a 128-B node holds four) — stats mode */
    uint64_t tris_tested;          /* triangles tested (48 B each)  — stats mode */
    uint64_t dropped_samples;      /* non-finite samples dropped                 */
    uint64_t iterations;           /* wavefront iterations launched              */
    double   trace_ms;             /* HIP-event time inside the trace kernel     */
    double   shade_ms;             /* HIP-event time inside the shade kernel     */
    uint64_t trace_launches;
    uint64_t bvh_nodes;            /* 4-wide inner nodes (128 B each)            */
    uint64_t bvh_bytes;            /* nodes + leaf triangles resident in HBM     */
    uint32_t bvh_max_depth;
    uint32_t scene_in_lds;         /* 0 BVH in HBM, 1 BVH staged in LDS, 2 tiny scene: all triangles tested (scalar loads) */
    uint64_t max_boxes_per_ray;    /* most child boxes a single closest-hit ray tested — stats mode */
    uint64_t parked_rays;          /* rays a trace launch handed on to the next one unfinished — stats mode */
    double   bvh_build_ms;         /* scene_create's BVH build: host wall time (SAH) or HIP-event time (LBVH) */
    uint32_t bvh_builder;          /* PATHED_BVH_* the scene was built with                 */
    uint32_t trace_launches_all;   /* trace launches since reset_stats, timed or not (trace_launches counts the timed ones) */
    uint32_t path_kernel;          /* 1 wavefront with the per-slot shade kernel, 2 wavefront with the staged shade kernel,
                                      3 fused path kernel (tiny scenes: one persistent launch per pass, timed as trace_ms),
                                      4 volume path kernel (PATHED_INTEGRATOR_VOLUME_PATH_TRACER),
                                      5 wavefront with the split shade stage (k_vertex + k_regen over the trace kernel's lists),
                                      6 wave path kernel (BVH scenes, the last render call),
                                      7 hybrid path kernel (scenes of 65 .. 4096 triangles, the last render call),
                                      8 feature kernel (the last call was pathed_hip_render_features[_device], or a render call
                                        of PATHED_INTEGRATOR_ALBEDO; its samples count in camera_samples and closest_rays),
                                      9 multiple-scattering volume kernel (PATHED_INTEGRATOR_BASIC_VOLUME),
                                      10 wavefront of an instanced scene (k_trace_instanced + k_shade_instanced),
                                         11 on such a scene while a shutter is set (pathed_hip_scene_set_instance_motion:
                                         k_trace_instanced_motion + k_shade_instanced_motion; the other meaning of 11 below
                                         cannot occur on the same scene: a scene with instances holds no medium),
                                      11 anisotropic multiple-scattering volume kernel (PATHED_INTEGRATOR_BASIC_VOLUME on a scene
                                         with a Henyey-Greenstein medium, pathed_hip_scene_set_medium_phase) */
    uint32_t reserved0;
    uint64_t local_closest_rays;   /* closest-hit queries the shade kernel resolved itself (rays that cannot meet anything but the
                                      scene's few large triangles, PathedSceneOptions.local_rays) -- stats mode; NOT in closest_rays */
    uint64_t local_shadow_rays;    /* ... and any-hit queries -- stats mode; NOT in shadow_rays */
} PathedStats;

/* ---- life cycle ---------------------------------------------------------- */

/* Select the device this process renders on (one process per GPU).
 * Replaces the reference's rtcNewDevice / rtcNewScene (app/main.cpp:46-52). */
int pathed_hip_init(int device_id);

/* Which builder stands in for rtcCommitScene (reference src/scene.cpp:39): PathedSceneOptions.bvh_builder:
 *   PATHED_BVH_SAH_HOST     binned-SAH tree built on the host cores (default: cheapest to traverse)
 *   PATHED_BVH_LBVH_DEVICE  Morton-code linear BVH built on the GPU in milliseconds;
 *                           same node format, so hits and images are bit-identical, traversal costs more.
 *   PATHED_BVH_PLOC_DEVICE  bottom-up clustering along the Morton order on the GPU (PLOC): a few times
 *                           the LBVH's build time, tree quality close to the SAH build's.
 * Meshes of <= 64 triangles always take the host path (they are not traversed at all). */
#define PATHED_BVH_SAH_HOST    0
#define PATHED_BVH_LBVH_DEVICE 1
#define PATHED_BVH_PLOC_DEVICE 2

/* Flatten + upload once: leaf-ordered 48-B triangles, flattened 4-wide BVH (128-B nodes),
 * spheres, material table, light table, env map + CDFs, camera.
 * Replaces rtcCommitScene (reference src/scene.cpp:39) and the light list
 * construction (src/scene_parser.cpp:173-190). */
int pathed_hip_scene_create(const PathedSceneDesc *desc, PathedScene **out);
void pathed_hip_scene_destroy(PathedScene *scene);

/* Refit: new vertex positions -- and optionally normals -- over an UNCHANGED topology, what
 * rtcCommitScene (reference src/scene.cpp:39) repeats for a deforming mesh.  The tree keeps its shape: leaf triangle
 * records, shading records and every node's child boxes are recomputed bottom-up on the device (milliseconds for millions
 * of triangles), boxes padded as the builders pad them.  positions: 3 * n_vertices floats, normals: the same or NULL (keep),
 * host memory; n_vertices must be the scene's.  device_ms (may be NULL): HIP-event time of the refit kernels, uploads excluded.
 * Needs PathedSceneOptions.refittable at creation; PATHED_E_UNSUPPORTED for scenes of <= 64 triangles (recreate those). */
int pathed_hip_scene_refit(PathedScene *scene, const float *positions, const float *normals, uint32_t n_vertices, float *device_ms);

/* Per-scene options.  Zero-initialise, set struct_size = sizeof(PathedSceneOptions), then set only
 * what you need: every field's "automatic" value is 0 except where stated, so a zeroed struct
 * means "all defaults" -- EXCEPT `device`, where 0 is device 0; use PATHED_DEVICE_CURRENT (-1) for
 * the device of pathed_hip_init.  The device is part of the scene: every call that takes the
 * PathedScene selects it first (hipSetDevice is per host thread), so a host may drive several
 * scenes on several GPUs from one thread per GPU (reference app/main.cpp:93-98 runs the
 * integrator on its own std::thread).  This struct is the ONLY way to tune the product library: it
 * reads no PATHED_* environment variable that could change a kernel, a slot count or a builder
 * (the experiments build, `make experiments`, still honours them for A/B scripts; two debug prints,
 * PATHED_DEBUG_ALLOC and PATHED_DEBUG_STATS, exist in both and change no result). */
#define PATHED_DEVICE_CURRENT (-1)
typedef struct PathedSceneOptions {
    uint32_t struct_size;       /* sizeof(PathedSceneOptions)                                  */
    int32_t device;             /* HIP device id, or PATHED_DEVICE_CURRENT                     */
    int32_t bvh_builder;        /* PATHED_BVH_* + 1 (0 = PATHED_BVH_SAH_HOST)                  */
    int32_t stack_rows;         /* LDS rows of the traversal stack: 8, 16 or 22 (0 = by tree depth); deeper entries spill to HBM */
    int32_t pools;              /* independent slot pools, 1..4 (0 = 2)                        */
    int32_t suspend_lanes;      /* park a trace wave's tail below this many rays, 1..64; -1 = never (0 = 32) */
    int32_t suspend_patience;   /* ... after this many steps without a new card, >= 1; -1 = none (0 = 24)     */
    int32_t park_min_cards;     /* ... while the pool has this many cards per wave, >= 1; -1 = always (0 = 1)  */
    int32_t max_slots;          /* path slots (0 = 1 Mi for all-triangles scenes; BVH scenes 8 Mi, fewer for short calls) */
    int32_t intersector;        /* 0 automatic, 1 always walk the BVH (never the all-triangles kernel)         */
    int32_t trace_blocks_per_cu;/* persistent trace blocks per CU (0 = automatic)              */
    int32_t shade_kernel;       /* 0 automatic; 1 wavefront, k_shade (one lane per slot); 2 wavefront, k_shade_staged (dense,
                                   state-sorted stages per block); 3 k_path_small (fused: whole paths in registers; scenes of
                                   <= 64 triangles only, their default); 4 wavefront, k_vertex + k_regen over the hit / miss
                                   lists the trace kernel writes (BVH scenes only); 5 k_path_wave (BVH scenes of <= 96 materials:
                                   paths in registers, the wave's rays shared through LDS, no path state in HBM) for every call.
                                   6 k_path_hybrid (sphere-free scenes of 65 .. 4096 triangles, <= 96 materials: the <= 64 largest
                                   triangles through the all-items intersector, the rest through a tree of their own, paths in
                                   registers).
                                   0 on a BVH scene: k_path_hybrid where it applies; else k_path_wave for calls of fewer than 48 Mi
                                   camera samples, whose rate hardly depends on the call's size, the wavefront (1) for longer ones
                                   (trees of up to 36 KB, which the wavefront would copy into LDS: k_path_wave at every length);
                                   images are identical */
    int32_t stage_slots;        /* slots per block of the staged kernel: 512 or 1024 (0 = automatic)           */
    int32_t unit_order;         /* order work units are handed out in (scheduling only, results identical):
                                 * 0 automatic = 1; 1 chunk stripes, rows; 2 chunk stripes, 32 x 8 tiles; 3 pixel tiles */
    int32_t build_threads;      /* host threads of the SAH builder (0 = all cores; the tree does not depend on it) */
    int32_t generic_kernels;    /* 1: never pick a scene-specialised kernel instantiation (k_shade<.., ENV_ONLY> for scenes whose
                                   one light is the environment and whose materials do not emit): A/B runs and tests */
    int32_t node_format;        /* the tree the trace kernel walks: 0 automatic; 1 128-byte nodes (four float boxes); 2 compressed
                                   64-byte nodes (the boxes on an 8-bit grid over their union, rounded outward: same hits);
                                   3 compressed 8-wide nodes (128 bytes, up to eight children: grandchildren pulled up) --
                                   2 and 3: sphere-free scenes whose tree stays in HBM, per-slot pipeline; an error elsewhere */
    int32_t small_phase1;       /* the fused kernel's conservative all-triangles pass (phase 1 of rtcIntersect1 / rtcOccluded1,
                                   reference src/scene.cpp:113,374): 0 automatic; 1 on the VALU (packed Moeller-Trumbore);
                                   2 on the matrix pipe (v_mfma_f32_32x32x2_f32 over Pluecker rows, mfma_candidates.h) --
                                   phase 2 decides either way: hits and images are bit-identical */
    int32_t refittable;         /* 1: keep the triangle soup (positions, normals, uvs, indices: 44 bytes per triangle or so) on the
                                   device so that pathed_hip_scene_refit can move the vertices later; BVH scenes only */
    int32_t wave_max_ksamples;  /* shade_kernel 0 on a BVH scene: render calls of fewer than this many x 1024 camera samples run
                                   k_path_wave, longer ones the wavefront (0 = 49 152, i.e. 48 Mi samples) */
    int32_t wave_stragglers;    /* k_path_wave / k_path_hybrid: a traversal burst ends once the wave's list is dealt and fewer rays
                                   than this are still in flight, 1..64; -1 = every ray is finished first (0 = 24 / 16).  Scheduling only */
    int32_t wave_refill;        /* k_path_wave / k_path_hybrid: idle lanes draw from the wave's ray list once fewer than this many are
                                   busy, 1..64 (0 = 48 / 40).  Scheduling only */
    int32_t chunks_per_pass;    /* work units per pixel of one internal pass, 1..4096 (0 = 256, fewer at resolutions whose partial
                                   sums would not fit): longer passes amortise a pass's ramp-up and drain, at 16 bytes per unit */
    int32_t local_rays;         /* the wavefront's local rays: a sphere-free BVH scene with at most 8 LARGE triangles (each >= 1 / 256 of
                                   its surface: a floor, a backdrop) lets the shade kernel resolve the rays that cannot meet the
                                   bounds of everything else -- they skip the trace kernel; same hits.  0 automatic (on), 1 off */
    int32_t shade_chain;        /* environment-lit scenes: the shade kernel that ends a sample starts the next one at once and, when its
                                   camera ray is a local ray that hits a large triangle, shades its first vertex in the same launch
                                   (k_shade_env).  0 automatic (on), 1 off.  Scheduling only */
    int32_t shade_launches;     /* ... shade launches per trace launch on such a scene, 1..16 (0 = 1: more were measured and lose): in the further ones the slots
                                   whose rays were all local advance another vertex, the others wait for the trace kernel, which
                                   then finds the tree-walking rays of several vertices in one launch.  Scheduling only */
    int32_t hybrid_batch;       /* k_path_hybrid: a wave walks its tree part once this many of its rays wait or are in flight,
                                   1..128 (1 = in every iteration; 0 = 24).  Scheduling only */
    int32_t hybrid_ready;       /* ... or once fewer of its paths than this can go on without a result, 1..64; -1 = only when
                                   none can (0 = 28).  Scheduling only */
} PathedSceneOptions;
int pathed_hip_scene_create_ex(const PathedSceneDesc *desc, const PathedSceneOptions *options, PathedScene **out);
int pathed_hip_scene_device(const PathedScene *scene);   /* the HIP device the scene lives on, or a negative error */

/* Instanced geometry -- the reference's "instance" / "instanced" models (src/scene_parser.cpp:231-249, 279-285, 449-492, which
 * hands them to Embree as RTC_GEOMETRY_TYPE_INSTANCE): a PROTOTYPE is a run of mesh geoms of the description that is not
 * placed in the world, an INSTANCE is one prototype under an affine transform.  One level: a host resolves nesting.
 *
 * Layout of the description: the mesh geoms cover the triangles in order without gaps; the world's geoms come first
 * (triangles [0, T0)), then the prototypes' geoms, prototype after prototype, to the end of the geom array.  A prototype's
 * vertices are in ITS space.
 *
 * Primitive ids are VIRTUAL: world triangles keep [0, T0); instance k owns [base_k, base_k + T_prototype(k)) in instance
 * order, base_0 = T0.  These are the ids of the FLATTENED scene -- every placement written out as world triangles in that
 * order by the flatten routine below -- so the acceptance rule "smaller t, then smaller primitive id" is the flattened
 * scene's, pathed_hip_trace reports them, and every shading quantity of a hit equals what the flattened scene's records
 * give for the same (t, u, v, prim).  The total must stay below 2^31 (PATHED_E_INVALID otherwise).
 *
 * The flatten routine (fp32, one rounding per operation, no fused multiply-add), with m = transform:
 *   point   x' = ((m[0] x + m[1] y) + m[2] z) + m[3]      y', z' from m[4..7], m[8..11]
 *   normal  x' = ((i[0] x + i[4] y) + i[8] z)             y' from i[1], i[5], i[9]; z' from i[2], i[6], i[10]   (not renormalised)
 * where i is the inverse of m, formed in double from the floats of m by cofactors -- c00 = e k - f h, c01 = c h - b k,
 * c02 = b f - c e, c10 = f g - d k, c11 = a k - c g, c12 = c d - a f, c20 = d h - e g, c21 = b g - a h, c22 = a e - b d for
 * m's 3 x 3 part (a b c / d e f / g h k), det = (a c00 + b c10) + c c20, i3x3 = c / det, translation -((r0 tx + r1 ty) + r2 tz)
 * per row -- and rounded once to float (pathed_amd/csrc/instances.h: instanceInverse).  pathed_amd.flatten_instances is this
 * routine in numpy.
 *
 * Memory: per instance one 112-byte record; nodes, leaf triangles and shading records exist once per prototype.
 * Such a scene renders on the wavefront with k_trace_instanced / k_shade_instanced whatever its size (PathedStats.path_kernel
 * 10); render, render_moments, select_pixels and render_pixels work as on every scene.
 *
 * PATHED_E_UNSUPPORTED, by name and before anything is allocated or launched: sphere primitives; media and passthrough
 * (container) materials; an emissive material inside a prototype (a host bakes such faces into world triangles, one copy per
 * placement); PathedSceneOptions.refittable; the device BVH builders; a shade_kernel other than 0 / 1.  On the created scene:
 * pathed_hip_scene_refit, every integrator but the path tracer, pathed_hip_render_features[_device],
 * pathed_hip_debug_small_candidates and pathed_hip_debug_light_records. */
typedef struct PathedPrototype {
    int32_t first_geom;      /* index into PathedSceneDesc.geoms */
    int32_t n_geoms;         /* >= 1, mesh geoms with at least one triangle together */
} PathedPrototype;
typedef struct PathedInstance {
    int32_t prototype;       /* index into PathedInstanceDesc.prototypes */
    float transform[12];     /* row-major 3 x 4, prototype space -> world; invertible */
} PathedInstance;
typedef struct PathedInstanceDesc {
    uint32_t struct_size;    /* sizeof(PathedInstanceDesc) */
    uint32_t n_prototypes;
    const PathedPrototype *prototypes;
    uint32_t n_instances;
    const PathedInstance *instances;
} PathedInstanceDesc;
int pathed_hip_scene_create_instanced(const PathedSceneDesc *desc, const PathedSceneOptions *options,
                                      const PathedInstanceDesc *instances, PathedScene **out);

/* Moving placements: new transforms for ALL instances of a scene made by pathed_hip_scene_create_instanced, what the reference
 * repeats rtcCommitScene for (src/scene.cpp:39), without building a prototype's tree or uploading a record again.
 * transforms: 12 floats per instance, row-major 3 x 4, in instance order -- the meaning of PathedInstance.transform; host
 * memory, or for the _device form memory on the scene's device (a simulation's tensor).  The host form uploads into a staging
 * buffer and runs the device form's code: there is one compute path.  n_instances must be the scene's; every instance's
 * prototype, the instance count, the virtual id bases and the prototypes stay as they are.
 *
 * On the device, k_instance_records restates every 112-byte record -- the inverse by the routine above, the same bits as the
 * host's -- into a second record buffer, and k_refit_top_pass refits the TOP tree bottom-up around the new world boxes (the
 * box rule of scene creation, pathed_amd.instances.placement_box in numpy).  The tree keeps its SHAPE: hits, ids and shading
 * are those of a scene created with the new transforms, but placements scattered far from where the tree was built make it
 * slower to walk (boxes of siblings overlap) -- a caller who moves them that far follows up with
 * pathed_hip_scene_rebuild_top below.  No prototype
 * node and no leaf triangle is written; the traversal stack's bound is unchanged.
 *
 * Order: the call first waits for ALL work on the scene's device (hipDeviceSynchronize), so render calls still running --
 * the *_device calls on a caller's stream included -- finish on the old tree, and a d_transforms that the caller's own stream
 * is still writing is complete; it returns once the device holds the new records and tree, so every later call, on any
 * stream, sees them.  Like pathed_hip_scene_refit it must not run concurrently with another call on the same scene.
 * device_ms (may be NULL): HIP-event time of the kernels, uploads excluded.
 *
 * PATHED_E_UNSUPPORTED: a scene without instances.  PATHED_E_INVALID: a null pointer, a count that is not the scene's, a
 * transform that is not finite or not invertible or whose inverse is not finite (the rule of scene creation; the message
 * names the lowest such instance index).  On every error the scene is exactly as it was before the call. */
int pathed_hip_scene_set_instance_transforms(PathedScene *scene, const float *transforms, uint32_t n_instances, float *device_ms);
int pathed_hip_scene_set_instance_transforms_device(PathedScene *scene, const float *d_transforms, uint32_t n_instances, float *device_ms);
/* Rebuilding the top tree: a NEW top tree over the scene's world triangles and its placements' CURRENT world boxes, built on
 * the device, in place of the one the scene was created with -- the other half of what the reference repeats rtcCommitScene
 * for.  Meant to follow pathed_hip_scene_set_instance_transforms when the placements were scattered far (a refitted tree keeps
 * its shape and gets slow to walk); valid on a scene that was never moved as well.  builder: PATHED_BVH_LBVH_DEVICE or
 * PATHED_BVH_PLOC_DEVICE.  The prototypes' trees, shading records and the render state stay; hits, ids and shading are those
 * of a scene created with the current transforms (hits do not depend on the tree).  A later set_instance_transforms refits
 * the new tree.  PathedStats.bvh_nodes / bvh_bytes / bvh_max_depth report the new tree, bvh_builder keeps saying what the
 * scene was created with.  With fewer than two primitives (world triangles + placements) there is nothing to arrange: the
 * call returns PATHED_OK and leaves the tree alone.
 *
 * Order: as pathed_hip_scene_set_instance_transforms -- the call first waits for all work on the scene's device and returns
 * synchronised; it must not run concurrently with another call on the same scene.  device_ms (may be NULL): HIP-event time
 * of the device work (the builder's, which includes its waits for a few counters, and the kernels around it).
 *
 * PATHED_E_INVALID: a null scene.  PATHED_E_UNSUPPORTED: a scene without instances; PATHED_BVH_SAH_HOST or an unknown
 * builder (the host builder needs the scene created again).  PATHED_E_DEVICE: an allocation or a kernel failed.  The new
 * arrays are built beside the live ones and adopted at the end: on every error the scene is exactly as it was. */
int pathed_hip_scene_rebuild_top(PathedScene *scene, int32_t builder, float *device_ms);
/* The shutter: placements that MOVE while a sample is taken.  transforms_close: 12 floats per instance, ALL instances, row-major
 * 3 x 4, the placements at shutter time 1; the scene's current transforms are the placements at time 0.  Host memory, or for
 * the _device form memory on the scene's device; one compute path, as above.  0 <= shutter_open <= shutter_close <= 1.
 *
 * The rule (pathed_amd/csrc/instances.h, pathed_amd.instances in numpy):
 *   transform at time t   m[i] = ((1 - t) * a[i]) + (t * b[i]) for the 12 floats a (time 0) and b (time 1), fp32, one rounding
 *                         per operation, no fused multiply-add (interpolateTransform); its inverse by the routine above
 *   time of a sample      t = open + (close - open) * u in fp32, u the sample's stream u(seed, pixel, sample, .) at dimension
 *                         0xFFFFFFFF (sampleTime) -- a dimension no vertex owns, so the camera jitter and every BSDF and light
 *                         number are the ones a scene without motion draws, and a pure function of (seed, pixel, sample), so any
 *                         split into calls, sample ranges, ranks or pixel lists draws the same times
 *   same transform twice  a placement whose a and b are bit-equal does not move: it keeps its record and its static box and is
 *                         walked and shaded as in a scene without motion, so a scene pays for the placements that move
 *   box                   a moving placement's world box is the union of its boxes at open and at close plus a pad
 *                         (movingPlacementBox: a point moves on a straight segment under a linearly interpolated matrix)
 *   singular in between   both END transforms must be finite and invertible; M(t) in between need not be (a half turn
 *                         interpolated linearly is singular at t = 0.5): a ray whose M(t) is not invertible, or whose inverse is
 *                         not finite, SKIPS that placement
 * Every sample of a render call then sees each moving placement at the sample's own time: a hit is what a scene created with
 * the transforms M(t) gives, bit for bit, in the walk and in shading.  With open == close every sample sees M(open).
 *
 * The call stores the second transforms, restates the moving placements' boxes (k_motion_boxes) and refits the top tree on the
 * device (k_refit_top_pass).  While motion is set the wavefront runs k_trace_instanced_motion / k_shade_instanced_motion and
 * PathedStats.path_kernel reports 11 on such a scene (10 without motion); the pixel-list calls work as on any instanced scene.
 * transforms_close == NULL removes the motion and restores the static boxes: renders are the static scene's bits again.
 * pathed_hip_scene_set_instance_transforms[_device] on a scene with motion replaces the time-0 transforms AND removes the
 * motion (the caller sets the motion of the next frame); pathed_hip_scene_rebuild_top builds over the moving boxes.
 * Order and device_ms: as pathed_hip_scene_set_instance_transforms.
 *
 * PATHED_E_UNSUPPORTED: a scene without instances.  PATHED_E_INVALID: a null scene, a count that is not the scene's, a shutter
 * outside 0 <= open <= close <= 1, a transform of time 1 that is not finite or not invertible.  All of it is refused before
 * anything is launched (the _device form finds a bad transform on the device, in one launch that writes beside the live state);
 * on every such refusal the scene is exactly as it was.  PATHED_E_DEVICE (a kernel of the refit failed): the scene keeps the
 * motion state it had -- it flips only after the refit succeeded -- but the top tree's boxes may be partly rewritten. */
int pathed_hip_scene_set_instance_motion(PathedScene *scene, const float *transforms_close, uint32_t n_instances,
                                         float shutter_open, float shutter_close, float *device_ms);
int pathed_hip_scene_set_instance_motion_device(PathedScene *scene, const float *d_transforms_close, uint32_t n_instances,
                                                float shutter_open, float shutter_close, float *device_ms);
/* Another view of the same scene: replaces the camera (reference Camera, src/camera.cpp:13-30) without rebuilding or
 * re-uploading anything; the resolution must stay (the caller's radiance sums are per pixel). */
int pathed_hip_scene_set_camera(PathedScene *scene, const PathedCamera *camera);

/* ---- the hot path -------------------------------------------------------- */

/* Render camera samples [spp_begin, spp_begin+spp_count) of every pixel and ADD
 * the per-pixel radiance sums into accum_rgb_sum (host memory, 3*W*H floats,
 * index 3*(row*W+col)+c, row 0 = bottom scanline) — exactly what
 * SampleIntegrator::sampleImage does to radianceLookup, spp_count times
 * (reference src/sample_integrator.cpp:61-63, src/integrator.cpp:42-51).
 * Bounce window as BounceController (reference src/bounce_controller.cpp:14-25);
 * last_bounce = -1 means unbounded, as in the reference (paths end on a miss or when the
 * throughput becomes exactly black). */
int pathed_hip_render(PathedScene *scene, uint64_t seed,
                      uint32_t spp_begin, uint32_t spp_count,
                      int start_bounce, int last_bounce,
                      float *accum_rgb_sum);

/* Same, but the sum buffer is DEVICE memory owned by the caller (e.g. a torch
 * tensor) and the work is enqueued on `stream` (a hipStream_t, NULL = default
 * stream).  The per-pixel sum CONTINUES from the buffer's current contents, so successive
 * calls whose lengths are multiples of the samples-per-unit setting are bit-identical to
 * one long call.  The call returns when the device work has completed (`blocking` is
 * reserved; the iteration loop polls a device counter). */
int pathed_hip_render_device(PathedScene *scene, uint64_t seed,
                             uint32_t spp_begin, uint32_t spp_count,
                             int start_bounce, int last_bounce,
                             float *d_accum_rgb_sum, void *stream, int blocking);

/* Which of the reference's SampleIntegrator subclasses the render calls run (job.json "integrator", src/job.cpp:65-97):
 *   PATHED_INTEGRATOR_PATH_TRACER         PathTracer::L (src/path_tracer.cpp:19-216), the default
 *   PATHED_INTEGRATOR_VOLUME_PATH_TRACER  VolumePathTracer::L (src/volume_path_tracer.cpp:14-131) with
 *                                         DirectLightingHelper::Ld (src/direct_lighting_helper.cpp:37-187): participating
 *                                         media behind PATHED_MAT_PASSTHROUGH containers, single scattering per segment.
 *   PATHED_INTEGRATOR_ALBEDO              AlbedoIntegrator::L (src/albedo_integrator.cpp:3-11): a sample is the first hit's emission
 *                                         (when the bounce window counts bounce 0 and the hit is no backside) plus
 *                                         Material::albedo -- a Lambertian's albedo lookup, (1, 0, 0) for EVERY other material, as
 *                                         in the reference (include/material.h:52-54) -- or the environment on a miss.  The render
 *                                         calls run the feature kernel: last_bounce is ignored, start_bounce only decides the
 *                                         emission, and a pixel's samples are summed one by one in sample order whatever
 *                                         pathed_hip_set_samples_per_unit says.
 *   PATHED_INTEGRATOR_BASIC_VOLUME        BasicVolumeIntegrator::L (src/basic_volume_integrator.cpp:25-197, src/job.cpp:73-74) with
 *                                         the same DirectLightingHelper::Ld: multiple scattering.  Every segment samples a
 *                                         scattering distance in the current medium (Medium::integrate); a path that scatters is
 *                                         weighted by the albedo (IntegrationResult::weight), lit there (VolumeHelper::
 *                                         directSampleLights, whatever the bounce window says) and turned through the isotropic
 *                                         phase function (include/phase.h, UniformSampleSphere, src/monte_carlo.cpp:43-52); the
 *                                         current medium is the top of a stack of the media the path has entered
 *                                         (updateMediumPtrs, :145-174; a surface without an internal medium pushes "none").  The
 *                                         stack holds four entries: a sample that would push a fifth is dropped and counted in
 *                                         PathedStats.dropped_samples.
 * Scenes that contain PATHED_MAT_PASSTHROUGH materials render with the two volume integrators only. */
#define PATHED_INTEGRATOR_PATH_TRACER 0
#define PATHED_INTEGRATOR_VOLUME_PATH_TRACER 1
#define PATHED_INTEGRATOR_ALBEDO 2
#define PATHED_INTEGRATOR_BASIC_VOLUME 3
int pathed_hip_set_integrator(PathedScene *scene, int integrator);

/* Summation granularity.  A pixel's samples are summed in sample order in groups of
 * `samples` (a work unit); the group sums are then added to the pixel in group order.
 * The result is deterministic for a given value.  The default, samples == 1, reproduces the
 * reference's order exactly (radianceLookup += one sample per wave, src/integrator.cpp:42-51);
 * it is also the finest grain of the work queue (a render call drains its last UNITS).
 * Larger groups write fewer partial sums (16 bytes per unit).  Range [1, 128]. */
int pathed_hip_set_samples_per_unit(PathedScene *scene, int samples);

/* First-hit feature images, rendered with the camera samples of the render calls (same seed, same sample indices: the ray
 * of pixel p, sample s is the render's): what a denoiser or a compositor wants beside the radiance sums.  Per sample whose
 * camera ray hits something in [1e-3, 1e5]:
 *   albedo_sum += the diffuse colour through the material's albedo kind (Lambertian, OrenNayar, Plastic), (1, 1, 1) for
 *                 Microfacet, Glass and Mirror
 *   normal_sum += the shading normal of the hit, world space, not flipped towards the viewer
 *   depth_sum  += t          hit_count += 1
 * and nothing on a miss.  A pixel's samples are added IN SAMPLE ORDER onto what the buffers hold, so any split of
 * [0, n) into calls gives the same floats.  The call follows pathed_hip_scene_set_camera and pathed_hip_scene_refit.
 * Scenes with PATHED_MAT_PASSTHROUGH materials: PATHED_E_UNSUPPORTED. */
typedef struct PathedFeatureBuffers {   /* device pointers; any may be NULL = not wanted (all NULL: PATHED_E_INVALID) */
    float *albedo_sum;   /* 3*W*H, layout of the radiance sums */
    float *normal_sum;   /* 3*W*H */
    float *depth_sum;    /* W*H   */
    float *hit_count;    /* W*H, samples that hit something (as float) */
} PathedFeatureBuffers;
/* buffers in DEVICE memory, work enqueued on `stream` (a hipStream_t, NULL = default stream); returns when it has completed */
int pathed_hip_render_features_device(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count,
                                      const PathedFeatureBuffers *buffers, void *stream);
/* buffers in HOST memory (any may be NULL); ADDS the call's samples to them like pathed_hip_render -- one by one, in sample
 * order, onto what they hold: 3 + 5 samples in two calls are the 8 of one call, bit for bit */
int pathed_hip_render_features(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count,
                               float *albedo, float *normal, float *depth, float *hits);

/* Per-pixel second moments: the render call that also keeps, beside the radiance sums, the per-channel sums of the SQUARED
 * sample colours -- the third thing a denoiser or an adaptive scheme wants, and what "render until the image is this clean"
 * is decided on.  The path kernels are the render calls' own: with one sample per unit every sample's colour has its own
 * entry in the pass's unit buffer, and the kernel that ends a pass adds a pixel's entries x to the sum and x * x (a multiply,
 * then an add) to the squares, in sample order.
 *   - d_rgb_sum gets exactly the floats pathed_hip_render_device would give.
 *   - both buffers (3*W*H floats, layout of the radiance sums) CONTINUE from their contents: any split of [0, n) into calls
 *     and internal passes gives the same floats.  A dropped (non-finite) sample adds zero to both.
 *   - PATHED_E_INVALID, and nothing is launched: a null buffer; a scene whose samples-per-unit is not 1 (a unit's entry is then
 *     the sum of a group of samples, and the last group of a call is ragged).
 *   - PATHED_E_UNSUPPORTED, and nothing is launched: PATHED_INTEGRATOR_ALBEDO, whose render calls run the feature kernel and
 *     have no unit buffer.
 * Precision: the squares are summed in fp32, as the radiance sums are.  The variance Q / n - m * m (below) cancels once a
 * pixel's relative noise falls below about 1e-3 -- far below any sensible target -- and is clamped at zero there. */
int pathed_hip_render_moments_device(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count,
                                     int start_bounce, int last_bounce,
                                     float *d_rgb_sum, float *d_rgb_sq_sum, void *stream);
/* buffers in HOST memory; ADDS the call's two sums to them like pathed_hip_render (the call's own sums start at zero) */
int pathed_hip_render_moments(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count,
                              int start_bounce, int last_bounce, float *rgb_sum, float *rgb_sq_sum);

/* The noise figure of an image from its two sum images over n_samples >= 2 samples per pixel.  Per pixel, with sums S_c,
 * square sums Q_c, n = (float)n_samples and a floor f > 0, all in fp32 and in this order (n and n / (n - 1) computed once):
 *     m_c = S_c / n
 *     d_c = Q_c / n - m_c * m_c          v_c = max(d_c, 0) * (n / (n - 1))
 *     e   = sqrt(((v_r + v_g) + v_b) / n) / (((m_r + m_g) + m_b) + f)
 * i.e. the standard error of the pixel's mean over its brightness; f keeps black pixels from dominating.  A non-finite e
 * counts as 0 and in invalid_pixels.  mean_error is the sum of e over the pixels in double -- per block of 256 pixels in
 * pixel order, the blocks in order: deterministic -- over W*H; max_error the largest e; pixels_above the pixels with
 * e > threshold.  d_error (W*H floats, device memory) receives e per pixel, or is NULL.  Device pointers live on the scene's
 * device; the work runs on `stream` (NULL = default stream) and the call returns when it has completed.
 * PATHED_E_INVALID: n_samples < 2, floor <= 0, out->struct_size != sizeof(PathedNoise), a null sum buffer or result. */
typedef struct PathedNoise {
    uint32_t struct_size;      /* sizeof(PathedNoise), set by the caller */
    uint32_t invalid_pixels;
    double   mean_error;
    double   max_error;
    uint64_t pixels_above;
} PathedNoise;
int pathed_hip_noise_estimate_device(PathedScene *scene, const float *d_rgb_sum, const float *d_rgb_sq_sum,
                                     uint32_t n_samples, float floor, float threshold,
                                     float *d_error, PathedNoise *out, void *stream);

/* Adaptive sampling: render only the pixels that are still noisy.  Beside the two sum images goes a COUNT image, W*H uint32
 * in device memory: the samples each pixel's sums hold.
 *
 * pathed_hip_select_pixels_device is pathed_hip_noise_estimate_device with n read per pixel from d_count: n = (float)count and
 * n / (n - 1) are computed per pixel, in fp32, and the formula above is applied operation for operation -- where every count
 * is the same n >= 2, e per pixel and every field of `out` are that call's bits.  A pixel with count < 2 has no spread yet:
 * its e counts as 0 and it counts in invalid_pixels.  The call also makes the list of the pixels still to render: those with
 * e > threshold and those with count < 2, as pixel indices (row * W + col) in ASCENDING order, written to d_list (room for W*H
 * uint32), their number to *n_list.  The list is built without atomics and is the same on every run.  d_error as above.
 * Returns when the work on `stream` has completed.  PATHED_E_INVALID: floor <= 0, struct_size, a null buffer, list or result.
 *
 * pathed_hip_render_pixels_device renders samples [spp_begin, spp_begin + spp_count) of the n_list pixels of d_list and
 * nothing else: the work units of its passes walk the list instead of the image (whatever PathedSceneOptions.unit_order
 * says), and the call splits into internal passes like every render call.  A list call runs on the path tracer's WAVEFRONT
 * kernels (PathedStats.path_kernel 1) whatever kernel the scene's other calls run on -- the fused, hybrid and wave kernels
 * do not know the list order (pathed_amd/csrc/kernels.h says why) -- which gives the same floats: all of them do.  A scene
 * whose calls run the volume integrators' kernels has a list form of those (k_list_volume; path_kernel 4 / 9 as ever).
 *   - a listed pixel's sums and square sums CONTINUE exactly as pathed_hip_render_moments_device would continue them over
 *     the same sample range -- the same floats, on every kernel organisation -- and its count grows by spp_count: a pixel
 *     that stops at n samples holds exactly the n-sample render's value.
 *   - no other pixel's entry of the three buffers is written or read.
 *   - n_list == 0 (or spp_count == 0): nothing is launched, PATHED_OK.
 *   - PATHED_E_INVALID, and nothing is rendered: a null buffer; a scene whose samples-per-unit is not 1; a list that is not
 *     strictly ascending (so: no pixel twice) or holds an index >= W*H -- a kernel checks the list before anything else runs.
 *   - PATHED_E_UNSUPPORTED, and nothing is launched: PATHED_INTEGRATOR_ALBEDO. */
int pathed_hip_select_pixels_device(PathedScene *scene, const float *d_rgb_sum, const float *d_rgb_sq_sum, const uint32_t *d_count,
                                    float floor, float threshold, float *d_error, uint32_t *d_list, uint32_t *n_list,
                                    PathedNoise *out, void *stream);
int pathed_hip_render_pixels_device(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count,
                                    int start_bounce, int last_bounce, const uint32_t *d_list, uint32_t n_list,
                                    float *d_rgb_sum, float *d_rgb_sq_sum, uint32_t *d_count, void *stream);

/* Heterogeneous media: the reference's GridMedium (src/grid_medium.cpp), a voxel grid of extinction densities that is
 * looked up trilinearly and walked cell by cell (pathed_amd/csrc/grid_medium.h).  PathedSceneDesc and PathedMedium do not
 * know it: a grid is set on a medium slot of a CREATED scene.
 *   cells_*          grid points per axis, each >= 2 (UniformGrid; cells_x * cells_y * cells_z < 2^31)
 *   bounds           min x, y, z, max x, y, z of the grid's box in MODEL space (the .vol file's order), max > min
 *   data             cells_x * cells_y * cells_z floats, index = (z * cells_y + y) * cells_x + x; host memory, copied
 *   albedo, scale    GridMedium's: sigma_t = density * scale, sigma_s = sigma_t * albedo
 *   world_to_model   row-major 4x4 and its inverse (the scene file's "transform" is model_to_world)
 * pathed_hip_scene_set_grid_medium turns medium slot `medium_index` into a grid medium (its sigma_t / sigma_s are ignored
 * from then on); called again on the same slot it replaces the grid.  It uploads the grid and rebuilds nothing else.
 * PATHED_E_INVALID: index out of range or a scene without media, cells < 2, bounds or data not finite, struct_size wrong.
 * A scene with a grid renders as PATHED_INTEGRATOR_VOLUME_PATH_TRACER or PATHED_INTEGRATOR_BASIC_VOLUME only; every other
 * render or feature call returns PATHED_E_UNSUPPORTED. */
typedef struct PathedGridMedium {
    uint32_t struct_size;   /* sizeof(PathedGridMedium) */
    uint32_t cells_x, cells_y, cells_z;
    float bounds[6];
    const float *data;
    float albedo;
    float scale;
    float world_to_model[16];
    float model_to_world[16];
} PathedGridMedium;
int pathed_hip_scene_set_grid_medium(PathedScene *scene, int medium_index, const PathedGridMedium *grid);

/* Test hook onto the grid code: for each of n segments (a, b: n * 3 floats each, world space, host memory) one thread runs
 * GridMedium::transmittance(a, b) and GridMedium::findTransmittance(a, b, target) on the grid of medium slot `medium_index`:
 * transmittance[i], and distance[i] (-1 where the reference's result is invalid). */
int pathed_hip_grid_queries(PathedScene *scene, int medium_index, size_t n, const float *a, const float *b, const float *target,
                            float *transmittance, float *distance);

/* Test hook onto the shading functions (BSDF evaluation and sampling, Fresnel, sphere and environment sampling), below the
 * image: one thread per record runs ONE function as the path kernels call it, in the instantiation `traits` of the kernels'
 * compile-time scene sets.  Records are fp32, host memory, in the layouts of tests/golden/README.md
 * (material(20) = type, albedo type, diffuse(3), emit(3), checker on(3), off(3), res(2), sigma, alpha, ior, distribution;
 *  isect(11) = geometric normal(3), shading normal(3), wo(3), uv(2)); the random numbers a sampling function draws are the
 * record's own u, in drawing order:
 *   function                          in                               out
 *   PATHED_QUERY_MATERIAL_F           material(20) isect(11) wi(3)     f(3) pdf
 *   PATHED_QUERY_MATERIAL_SAMPLE      material(20) isect(11) u(3)      wi(3) pdf throughput(3)
 *   PATHED_QUERY_FRESNEL              cos etaI etaT                    F
 *   PATHED_QUERY_SPHERE_SAMPLE        center(3) radius ref(3) u(2)     point(3) normal(3) invPDF measure (0 solid angle, 1 area)
 *   PATHED_QUERY_SPHERE_PDF           center(3) radius ref(3)          solid-angle pdf
 *   PATHED_QUERY_ENV_EMIT             lightWo(3)                       Le(3)
 *   PATHED_QUERY_ENV_PDF              direction(3)                     pdf, thetaStep, phiStep, thetaPDF * phiPDF * width * height
 *   PATHED_QUERY_ENV_SAMPLE           point(3) u(2)                    point(3) normal(3) invPDF thetaStep phiStep
 * The environment functions run on the scene's environment; nothing else of the scene is read.
 * PATHED_E_INVALID, and nothing is launched: a material type, distribution or albedo kind outside the set `traits` (image
 * textures and the passthrough material in every set), a sphere function on a set without spheres, an environment function
 * on a set without environment or a scene without one, u outside [0, 1], a zero or non-finite environment direction. */
enum {
    PATHED_QUERY_MATERIAL_F = 0, PATHED_QUERY_MATERIAL_SAMPLE = 1, PATHED_QUERY_FRESNEL = 2, PATHED_QUERY_SPHERE_SAMPLE = 3,
    PATHED_QUERY_SPHERE_PDF = 4, PATHED_QUERY_ENV_EMIT = 5, PATHED_QUERY_ENV_PDF = 6, PATHED_QUERY_ENV_SAMPLE = 7
};
enum {
    PATHED_TRAITS_ALL = 0, PATHED_TRAITS_LAMBERTIAN_TRIANGLES = 1, PATHED_TRAITS_LAMBERTIAN_PLASTIC_SPHERES = 2,
    PATHED_TRAITS_LAMBERTIAN_GLASS_CONTAINER = 3, PATHED_TRAITS_TRIANGLE_LIT = 4, PATHED_TRAITS_ENVIRONMENT_ONLY = 5,
    PATHED_TRAITS_ROUGH_BECKMANN = 6, PATHED_TRAITS_ROUGH_GGX = 7, PATHED_TRAITS_SMOOTH = 8, PATHED_TRAITS_COUNT = 9
};
int pathed_hip_debug_shading_queries(PathedScene *scene, int function, int traits, size_t n, const float *in, float *out);

/* Test hook onto the phase function of PATHED_INTEGRATOR_BASIC_VOLUME: the device's phaseSample (pathed_amd/csrc/volume.h =
 * UniformSampleSphere, src/monte_carlo.cpp:43-52), one thread per record, on scripted numbers instead of the path's stream.
 * u: n * 2 floats in [0, 1] (z's number, then phi's); out: n * 3 floats, the direction (r cos phi, z, r sin phi).  Host
 * memory both.  PATHED_E_INVALID, and nothing is launched: a number outside [0, 1], more than 2^20 records. */
int pathed_hip_debug_phase_samples(PathedScene *scene, size_t n, const float *u, float *out);

/* Anisotropic scattering: the Henyey-Greenstein phase function (pathed_amd/csrc/volume.h states value, sample, frame and
 * threshold).  PathedMedium does not know it: like a grid, a phase function is set on a medium slot of a CREATED scene,
 * homogeneous or grid; called again on the same slot it replaces the entry.  g > 0 scatters forward, along the direction the
 * path travels in.  A slot of type PATHED_PHASE_ISOTROPIC, one with |g| < 1e-3 and one never set scatter isotropically, with
 * the bits they always had.
 * A scene with at least one Henyey-Greenstein slot of |g| >= 1e-3 (whether or not a surface references the slot):
 *   - PATHED_INTEGRATOR_BASIC_VOLUME render calls (render, render_device, render_moments*) run the anisotropic kernels,
 *     PathedStats.path_kernel 11;
 *   - PATHED_INTEGRATOR_VOLUME_PATH_TRACER render calls and pixel-list renders (pathed_hip_render_pixels_device) under either
 *     volume integrator return PATHED_E_UNSUPPORTED, and nothing is launched.
 * PATHED_E_INVALID, and the scene is as it was: a null scene or pointer, a wrong struct_size, an index out of range (so: a
 * scene without media), an unknown type, g not finite or |g| > 0.99. */
enum { PATHED_PHASE_ISOTROPIC = 0, PATHED_PHASE_HENYEY_GREENSTEIN = 1 };
#define PATHED_PHASE_ISOTROPIC_BELOW 1e-3f   /* the threshold on |g| */
typedef struct PathedPhaseFunction {
    uint32_t struct_size;   /* sizeof(PathedPhaseFunction) */
    int32_t type;           /* PATHED_PHASE_* */
    float g;                /* mean cosine, |g| <= 0.99; ignored by PATHED_PHASE_ISOTROPIC (but checked) */
} PathedPhaseFunction;
int pathed_hip_scene_set_medium_phase(PathedScene *scene, int medium_index, const PathedPhaseFunction *phase);

/* Test hook onto that phase function, beside pathed_hip_debug_phase_samples: one thread per record calls the two functions
 * the anisotropic kernels call.  records: n * 9 floats (g, w(3), u1, u2, wi(3)) -- w the unit propagation direction, wi a unit
 * direction, u1 and u2 in [0, 1]; out: n * 4 floats, the direction sampled about w from (u1, u2), then p(w, wi).  Host memory
 * both.  Below the threshold the direction is pathed_hip_debug_phase_samples' and p is 1.f / fourPi.
 * PATHED_E_INVALID, and nothing is launched: |g| > 0.99, a number outside [0, 1] or not finite, more than 2^20 records. */
int pathed_hip_debug_phase_hg(PathedScene *scene, size_t n, const float *records, float *out);

/* Test hook onto the intersector that stands in for Embree.
 * rays: n * 8 floats (ox,oy,oz,tnear, dx,dy,dz,tfar), host memory.
 * any_hit == 0: closest hit (rtcIntersect1, reference src/scene.cpp:91-117):
 *               hits = n * 4 x 32-bit (t, u, v as float; prim as int32, -1 = miss;
 *               prim < n_triangles: triangle, else sphere n_triangles+i).
 * any_hit != 0: occlusion (rtcOccluded1, reference src/scene.cpp:355-381):
 *               hits = n * int32 (1 = occluded). */
int pathed_hip_trace(PathedScene *scene, const float *rays, size_t n,
                     int any_hit, void *hits);
/* ... with one shutter time per ray, on a scene with motion (pathed_hip_scene_set_instance_motion): the test hook of the
 * shutter, k_trace_rays_instanced_motion.  times: n floats inside the scene's shutter [open, close], host memory.  Ray i
 * meets every moving placement under the transform M(times[i]) of the rule stated there -- the hit, bit for bit, of a scene
 * created with those transforms -- and skips a placement whose M(times[i]) is not invertible.  PATHED_E_UNSUPPORTED: a
 * scene without instances.  PATHED_E_INVALID: a scene without motion, a null buffer, a time outside the shutter (the moving
 * boxes cover the shutter and nothing beyond it). */
int pathed_hip_trace_timed(PathedScene *scene, const float *rays, const float *times, size_t n,
                           int any_hit, void *hits);

/* Test hook onto phase 1 of the all-triangles intersector (scenes of <= 64 triangles; the stand-in for
 * rtcIntersect1 / rtcOccluded1 on such scenes, reference src/scene.cpp:113,374).
 * rays: n * 10 floats (origin.xyz, continuation direction.xyz, shadow direction.xyz, shadow tfar), host memory.
 * out:  n * 8 x uint64, bit p = ORIGINAL primitive id p (triangle ids of such scenes are < 64):
 *       candidates of the pair-of-triangles phase 1 (continuation, shadow), of the matrix-pipe phase 1 (continuation,
 *       shadow; zero in the product library), triangles phase 2 accepts (continuation: t in (1e-3, 1e5]; shadow: t in
 *       (1e-3, tfar]), candidates of the ITEM phase 1 the fused kernel runs -- parallelograms for the triangle pairs that
 *       form one (pathed_amd/csrc/small_items.h) -- (continuation, shadow).
 * Phase 1 is correct iff accepted is a subset of candidates for every ray. */
int pathed_hip_debug_small_candidates(PathedScene *scene, const float *rays, size_t n, uint64_t *out);

/* Test hook onto the shadow ray's phase 1 as the fused kernel runs it: the items that can never occlude a light sample
 * (pathed_amd/csrc/small_items.h: NEVER-OCCLUDERS) come last in item order and the shadow ray's pass stops before them.
 * rays: n * 10 floats as pathed_hip_debug_small_candidates takes them (the shadow ray is origin, shadow direction, shadow tfar).
 * out:  n * 2 x uint64, bit p = ORIGINAL primitive id p: the pruned item-form candidates of the shadow ray, the triangles
 *       phase 2 accepts for it (t in (1e-3, tfar]).  The pruning is correct iff accepted is a subset of candidates for every ray
 *       that sampleLightsTerm can build: from a point on a scene surface to a point on an emitter.
 * layout: 4 x int32: parallelograms, lone triangles, the shadow ray's turns over parallelogram pairs and over lone pairs.
 * never_occluders: one uint64, bit p = primitive p is a never-occluder.  Both are written even when n is 0. */
int pathed_hip_debug_shadow_candidates(PathedScene *scene, const float *rays, size_t n, uint64_t *out, int32_t *layout, uint64_t *never_occluders);

/* Test hook onto the PASS LIST of the fused kernel (pathed_amd/csrc/small_items.h: NEVER-HIT): the item list without the
 * triangles that are bit-for-bit copies of a triangle with a lower primitive id, as the non-counting parallelogram
 * instantiations walk it for a vertex's two rays -- its own records and counts, the shadow ray's turns pruned.  The hook
 * ALWAYS prunes the shadow ray; of the instantiations that take the list only the Cornell-like one does (kernels.h:
 * kSmallPrunes), the others run every turn for both rays: for those the hook's shadow word is a subset of the kernel's,
 * so a test that finds every accepted hit among the hook's candidates holds for the kernel all the more.
 * rays: n * 10 floats as pathed_hip_debug_small_candidates takes them.
 * out:  n * 2 x uint64, bit p = ORIGINAL primitive id p: the pass's candidates of the path ray, of the shadow ray.
 * primitives: n_triangles (the scene's triangle count) x int32: the primitive ids in pass order, -1 beyond the pass list.
 * layout: 5 x int32: parallelograms, lone triangles, the shadow ray's turns over parallelogram pairs and over lone pairs,
 *       triangles -- all of the pass list.
 * never_hit: one uint64, bit p = primitive p is left out of the pass.  The last three are written even when n is 0. */
int pathed_hip_debug_pass_candidates(PathedScene *scene, const float *rays, size_t n, uint64_t *out, int32_t *primitives, size_t n_triangles,
                                     int32_t *layout, uint64_t *never_hit);

/* Test hook onto the per-pixel candidate masks of the camera rays (scenes on the fused path kernel only; built at scene
 * creation and again by pathed_hip_scene_set_camera, pathed_amd/csrc/camera_masks.h).
 * out: n_pixels x uint64, row-major pixels, host memory; n_pixels must be width * height.  Bit 63 - k = triangle k of the
 *      ITEM order (the order phase 2 of the fused kernel indexes; pathed_hip_debug_item_order maps it to primitive ids).
 * The masks are correct iff, for every ray through a pixel's footprint, what phase 2 accepts is a subset of the pixel's mask. */
int pathed_hip_debug_camera_masks(PathedScene *scene, uint64_t *out, size_t n_pixels);

/* The item order of a scene of <= 64 triangles: primitives[k] = original primitive id of item-order triangle k.
 * n_triangles must be the scene's triangle count. */
int pathed_hip_debug_item_order(PathedScene *scene, int32_t *primitives, size_t n_triangles);

/* Test hook onto the records that hold per-triangle and per-light constants of the shading code (built on the device at scene
 * creation and again by a refit), next to what the per-vertex functions compute for the same triangles.
 * triangles: n_triangles * 20 floats, host memory, per primitive
 *       [0..3]   triangleSample's normal (xyz) and inverse pdf (the area)                   computed by the per-vertex functions
 *       [4..7]   trianglePdfSolidAngle's area pdf 1 / area; sampleLightsTerm's invPDF and 1 / invPDF for the scene's light count; -
 *       [8..11]  makeIsect's shading normal of a triangle without vertex normals (xyz); -
 *       [12..15] the shading record's (normal xyz, 1 / area) read where a BSDF sample meets an emitter      the stored records
 *       [16..19] the stored shading normal (xyz) of the plain-triangle record; -
 * lights:    room for max_lights * 18 floats; *n_lights lights are written, each as kind, primitive (as floats), then its 64-byte
 *       sampling record (p0, material bits) (p1, area) (p2, invPDF) (normal, 1 / invPDF); all zero for a light that is not a triangle.
 * n_triangles must be the scene's triangle count; more lights than max_lights is PATHED_E_INVALID. */
int pathed_hip_debug_light_records(PathedScene *scene, float *triangles, size_t n_triangles, float *lights, size_t max_lights, int *n_lights);

/* Test hook onto the placements' records as the device holds them (scene creation writes them on the host,
 * pathed_hip_scene_set_instance_transforms on the device): 28 words per instance, host memory -- the transform's rows (12
 * floats), the inverse's rows (12 floats), then four int32: virtual id base, prototype, the prototype's root node, its first
 * shading record.  n_instances must be the scene's.  PATHED_E_UNSUPPORTED on a scene without instances. */
int pathed_hip_debug_instance_records(PathedScene *scene, float *records /* 28 words per instance */, size_t n_instances);

/* 1 in libpathed_hip_experiments.so (`make experiments`), 0 in the product library.  The experiments build adds the
 * kernel organisations that were measured and rejected: shade_kernel 2 (staged) and 4 (split),
 * node_format 2 / 3 (compressed nodes), small_phase1 2 (matrix pipe) and pathed_hip_measure_valu_clocks; the product
 * library answers PATHED_E_UNSUPPORTED to each of them.  (pathed_hip_debug_small_candidates runs in both: the product reports
 * zero for the matrix-pipe form's two words.)  The experiments build also honours the PATHED_* tuning variables. */
int pathed_hip_has_experiments(void);

/* Bit 0: the counting variants of the trace kernel (nodes_visited / tris_tested); off by default, the
 * timed path never counts.  Bit 1: HIP-event pairs around every trace and shade launch (trace_ms,
 * shade_ms, trace_launches).  Bit 2: ... around every 8th launch only: the event pairs keep a pool's
 * kernels from running back to back and cost ~6 % of the rate when every launch is timed. */
int pathed_hip_set_stats_mode(PathedScene *scene, int enabled);
int pathed_hip_get_stats(PathedScene *scene, PathedStats *out);
int pathed_hip_reset_stats(PathedScene *scene);

/* Export the flattened BVH so a checker can walk the SAME tree.
 * nodes: 32 floats per 4-wide node, the four children in the components of
 *   (lo.x[4]) (lo.y[4]) (lo.z[4]) (hi.x[4]) (hi.y[4]) (hi.z[4]) (ref[4]) (unused);
 *   ref is an int32: >= 0 inner node index, <= -2 leaf with -ref - 1 =
 *   (first leaf triangle << 3) | triangle count, INT32_MIN empty slot.
 * tris: 12 floats per leaf triangle (v0.xyz, prim) (e1.xyz, -) (e2.xyz, -).
 * Pass NULL to query sizes. */
int pathed_hip_scene_export_bvh(PathedScene *scene,
                                float *nodes, size_t *n_nodes,
                                float *tris, size_t *n_tris);
/* The compressed form of the same nodes, same indices.
 * node_format 2, 16 words per node, same refs:
 *   (origin.xyz, scale.x) (scale.y, scale.z, qlo.x, qlo.y) (qlo.z, qhi.x, qhi.y, qhi.z) (ref[4])
 * node_format 3, 32 words per node, up to eight children (children of children pulled up; nodes no ref reaches are dead):
 *   (origin.xyz, scale.x) (scale.y, scale.z, qlo.x[2]) (qlo.y[2], qlo.z[2]) (qhi.x[2], qhi.y[2]) (qhi.z[2], -, -) (ref[0..3]) (ref[4..7]) (-)
 * origin / scale are floats, a q word holds four children's 8-bit grid indices (child c in bits 8(c mod 4) .. of word c / 4):
 * child c spans [origin + qlo * scale, origin + qhi * scale] per axis and CONTAINS its float box.
 * *n_nodes comes back 0 for a scene that does not carry a compressed form.  Pass NULL to query the sizes. */
int pathed_hip_scene_export_compressed_nodes(PathedScene *scene, uint32_t *nodes, size_t *n_nodes, size_t *words_per_node);

/* Measurement aid: what a plain streaming kernel reaches on THIS device, as a
 * second denominator beside the 8 TB/s HBM3E spec figure.  Allocates two probe buffers of `bytes`
 * (use >= 1 GiB: beyond the 256 MB Infinity Cache), times `repeats` passes of a 16-byte-per-lane
 * read kernel and of a copy kernel with HIP events.  read_gbs = bytes read / s; copy_gbs counts
 * bytes read + bytes written. */
int pathed_hip_measure_bandwidth(size_t bytes, int repeats, double *read_gbs, double *copy_gbs);

/* Measurement aid: the VALU issue rate THIS device sustains, in wave-instructions per second, as the
 * denominator of the "VALU issue" bound quoted for the scenes whose ray queries never leave the
 * registers (<= 64 triangles).  Runs `waves_per_simd` waves (1..8) on every SIMD of the chip, each
 * issuing `instructions_per_wave` INDEPENDENT v_fma_f32 (eight accumulator chains per lane, so no
 * wave ever waits on its own result), timed with HIP events over `repeats` launches.
 * fma_rate = v_fma_f32 wave-instructions / s (one VGPR source, scalar multiplier and addend); mixed_rate = the
 * same with one v_rcp_f32 / v_sqrt_f32 pair per six v_fma_f32 (what a path tracer's normalisations issue). */
int pathed_hip_measure_valu(int waves_per_simd, int repeats, double *fma_rate, double *mixed_rate);
/* The same probe over n_modes (<= 5) instruction mixes, rates[mode] in wave-instructions / s:
 * 0 v_fma_f32 with one VGPR source (scalar multiplier / addend: no register-bank conflicts), 1 six of those + v_rcp_f32 +
 * v_sqrt_f32, 2 v_fma_f32 with three VGPR sources, 3 v_pk_fma_f32 (two FMAs per lane), 4 v_mul_lo_u32. */
int pathed_hip_measure_valu_modes(int waves_per_simd, int repeats, double *rates, int n_modes);

/* The probe with its own clocks: `chains` (8 or 16) independent v_fma_f32 chains per lane on three VGPR operands; every
 * wave reads the shader clock (s_memtime) and the constant-rate wall clock (s_memrealtime) around its loop, so the issue
 * rate comes out in CYCLES PER INSTRUCTION at the frequency the chip actually ran at under this load, beside the rate
 * in instructions per second from HIP events.  (The guide's constants table has v_fma_f32 at 2 cycles per wave64
 * instruction: 1 228.8 G wave-instr/s at 2.4 GHz on 1 024 SIMDs.) */
typedef struct PathedValuClocks {
    double rate;                          /* wave-instructions / s, HIP events over `repeats` launches              */
    double shader_clock_mhz;              /* s_memtime ticks / s_memrealtime ticks x wall_clock_mhz                   */
    double wall_clock_mhz;                /* hipDeviceAttributeWallClockRate                                         */
    double peak_clock_mhz;                /* hipDeviceAttributeClockRate (what the device advertises)                */
    double wave_ticks_per_instruction;    /* shader-clock ticks one wave needs per instruction it issues             */
    double cycles_per_instruction;        /* ... divided by the waves that share its SIMD: the SIMD's issue interval */
    double cycles_per_instruction_events; /* SIMDs x shader clock / rate: the same from the event time               */
} PathedValuClocks;
int pathed_hip_measure_valu_clocks(int waves_per_simd, int chains, int repeats, PathedValuClocks *out);

/* ---- multi-GPU fan-in ------------------------------------------------------ */
/* The path's one exchange step: per-GPU radiance sums -> one buffer (the reference's
 * waves are additive, src/integrator.cpp:42-51).  A host that drives several scenes in one process
 * (one worker thread per GPU) uses these two instead of RCCL:
 *   pathed_hip_accum_copy_peer  copies `count` floats from src (on src_scene's device) into dst (on
 *                               dst_scene's device) over xGMI (hipMemcpyPeer); blocking.
 *   pathed_hip_accum_add        dst[i] += src[i] on dst_scene's device; blocking. */
int pathed_hip_accum_copy_peer(PathedScene *dst_scene, float *dst, PathedScene *src_scene, const float *src, size_t count);
int pathed_hip_accum_add(PathedScene *dst_scene, float *dst, const float *src, size_t count);
/* Device memory for such buffers, on the scene's device (hipMalloc / hipFree / hipMemcpy wrappers so a
 * plain C++ host needs no HIP headers). */
int pathed_hip_accum_alloc(PathedScene *scene, size_t count, float **out);   /* zero-filled */
int pathed_hip_accum_free(PathedScene *scene, float *buffer);
int pathed_hip_accum_download(PathedScene *scene, const float *buffer, size_t count, float *host);
int pathed_hip_accum_upload(PathedScene *scene, float *buffer, size_t count, const float *host);

/* The same exchange step as ONE collective: ncclReduce(sum, fp32, count, root = replica 0) over RCCL / xGMI
 * (the reference adds its waves in src/integrator.cpp:42-51).  A communicator spans the
 * devices of one process's replicas (ncclCommInitAll); librccl is loaded when the first communicator is made,
 * so a single-GPU host never pays for it.  Devices must be distinct (RCCL refuses two ranks on one device:
 * replicas that share a GPU use the peer-copy calls above); n_devices = 1 is a valid communicator.
 *   pathed_hip_comm_reduce  send[r] holds `count` floats on device_ids[r]; their sum lands in recv_root on
 *                           device_ids[0] (may equal send[0]: in place); blocking. */
typedef struct PathedComm PathedComm;
int pathed_hip_comm_init(int n_devices, const int *device_ids, PathedComm **out);
int pathed_hip_comm_reduce(PathedComm *comm, const float *const *send, float *recv_root, size_t count);
void pathed_hip_comm_destroy(PathedComm *comm);

const char *pathed_hip_last_error(void);
const char *pathed_hip_version(void);   /* "pathed_hip <version> (gfx950, abi <PATHED_ABI_VERSION>)" */

#ifdef __cplusplus
}
#endif
#endif /* PATHED_HIP_H */
