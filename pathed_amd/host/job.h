// job.json reader, reference include/job.h:13-75 + src/job.cpp:25-97.
// Same keys as the reference (spp, integrator, scene, startBounce, lastBounce,
// output_directory, output_name, showUI, force, width, height); job-file numbers are real
// JSON numbers.  Optional extra keys with defaults, so reference job files run unchanged:
//   "seed" (1): any integer in [0, 2^64), read exactly as written -- digits only: a negative, fractional or over-range value,
//               one written with an exponent and anything that is not a number are refused by name,
//   "gpu" (0), "asset_root" (directory paths resolve in),
//   "spp_per_launch" (1024): samples per render call.  A call drains its last paths before it returns (a few ms on a
//               BVH scene: 64 spp per call cost 4 %, 256 and more < 1 %); checkpoints still bound a call,
//   "bvh_builder" ("auto" | "sah" | "lbvh" | "ploc": include/pathed_hip.h PATHED_BVH_*; "auto" = the host SAH build on one
//               GPU, the device PLOC build when several GPUs each need the tree of a mesh of more than a million triangles:
//               N replicas would otherwise run N host builds side by side, seconds of serial time before the first sample),
//   "gpus" (1): a count N -> devices gpu .. gpu+N-1, or an explicit list of device ids (an id may
//               repeat: several replicas on one GPU); the samples of every batch are split over them,
//   "resume" (false): continue from <output_directory>/auto.state if it exists,
//   "features" (absent): a list out of "albedo", "normal", "depth" -- first-hit feature images of the same camera samples
//               (include/pathed_hip.h: pathed_hip_render_features), written beside every auto*.exr as auto-albedo*.exr,
//               auto-normal*.exr, auto-depth*.exr.  An unknown name is an error.
//   "target_noise" (absent): a number > 0.  The run keeps per-pixel second moments (include/pathed_hip.h:
//               pathed_hip_render_moments_device), estimates the image's noise figure -- the mean over the pixels of the standard
//               error of the pixel's mean over its brightness, pathed_hip_noise_estimate_device -- at the power-of-two checkpoints
//               from "min_spp" on, and stops at the first one at or below the target; "spp" stays the cap,
//   "min_spp" (16): an integer >= 2, the first sample count the figure is looked at,
//   "noise_floor" (0.01): a number > 0 added to a pixel's brightness in that ratio, so that black pixels do not dominate,
//   "stderr_image" (false; implied by "target_noise"): write the per-channel standard error of the mean as auto-stderr*.exr
//               beside every auto*.exr and record the figure in the log and in metrics.json ("noise", "stopped_on_noise").
//               Neither key goes with "resume": the state file holds no squares.  Bad values are refused by name.
//   "shutter" (absent = [0, 1]): [open, close] with 0 <= open <= close <= 1.  A scene file whose top-level "instanced" models
//               carry "transform_close" renders with those placements moving from "transform" (shutter time 0) to
//               "transform_close" (time 1): every sample sees them at its own time in [open, close] (include/pathed_hip.h:
//               pathed_hip_scene_set_instance_motion).  Refused by name on a scene where nothing moves,
//   "adaptive" (false; needs "target_noise"): render on only the pixels that are still noisy.  The schedule is fixed:
//                 1. min("min_spp", "spp") samples of every pixel (pathed_hip_render_moments_device);
//                 2. rounds: each selects, among the pixels still active, those whose OWN error e exceeds "target_noise"
//                    (pathed_hip_select_pixels_device) and takes them from n to min(2 n, "spp") samples
//                    (pathed_hip_render_pixels_device).  A pixel that was not selected has retired and stays retired: its sums,
//                    and so its e, no longer change.  All active pixels therefore share one count n;
//                 3. the run ends when no pixel is selected or n has reached "spp".
//               The criterion is PER PIXEL -- stricter than the image-mean criterion of a "target_noise" run without
//               "adaptive", which stops once the MEAN of e is at or below the target and leaves its noisiest pixels above it.
//               The image is sum / count per pixel.  Written beside auto*.exr and auto-stderr*.exr after the first step
//               and after every round: auto-spp*.exr, the count image (HALF: whole numbers are exact up to 2048, even ones up
//               to 4096, ..).  metrics.json gains "samples_rendered", "adaptive_rounds", "pixels_at_cap" (pixels that hold
//               "spp" samples), "uniform_spp" and "uniform_samples" (for comparison: the largest count, which a uniform render
//               held to the same per-pixel criterion would give EVERY pixel, and that times the pixels).  "adaptive" is refused by name beside "resume", more than one GPU and the
//               AlbedoIntegrator; sharding a pixel list over GPUs is not done.
#pragma once

#include "bounce_controller.h"
#include "json.h"

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace pathed {

class Integrator;

class Job {
public:
    explicit Job(const std::string &jobPath);
    explicit Job(const Json &json);

    // creates <output_directory>/ and writes report.json (src/job.cpp:33-63)
    void init();

    bool showUI() const { return m_json["showUI"].isBool() && m_json["showUI"].asBool(); }
    bool force() const { return m_json["force"].isBool() && m_json["force"].asBool(); }

    int width() const { return m_json["width"].asInt(); }
    int height() const { return m_json["height"].asInt(); }

    int spp() const
    {
        const int spp = m_json["spp"].asInt();
        return spp > 0 ? spp : 9999999;
    }

    std::string outputDirectory() const { return m_json["output_directory"].asString() + "/"; }
    std::string outputName() const { return m_json["output_name"].isString() ? m_json["output_name"].asString() : ""; }
    std::string scene() const { return m_json["scene"].asString(); }
    std::string integratorName() const { return m_json["integrator"].asString(); }

    int startBounce() const { return m_bounceController.startBounce(); }
    int lastBounce() const { return m_bounceController.lastBounce(); }
    BounceController bounceController() const { return m_bounceController; }

    // "seed": any integer in [0, 2^64), read exactly as written (Json::asUnsigned); anything else throws an error that names the key
    unsigned long long seed() const;
    int sppPerLaunch() const
    {
        if (!m_json["spp_per_launch"].isNumber()) { return 1024; }
        const double value = m_json["spp_per_launch"].asNumber();
        if (!(value >= 1.0) || value > 1e6) { throw std::runtime_error("job: spp_per_launch must be in [1, 1000000]"); }
        return (int)value;
    }
    bool resume() const { return m_json["resume"].isBool() && m_json["resume"].asBool(); }
    std::vector<int> devices() const;
    std::vector<std::string> features() const;   // in the order albedo, normal, depth
    // "target_noise" / "min_spp" / "noise_floor" / "stderr_image", validated (a bad value throws an error that names its key)
    struct NoiseSettings {
        double target = 0.0;   // 0 = none
        int minSpp = 16;
        double floor = 0.01;
        bool collect = false;  // a target or "stderr_image": the run keeps second moments
        bool adaptive = false; // "adaptive": pixel lists (needs a target)
    };
    NoiseSettings noise() const;
    // "shutter": [open, close] with 0 <= open <= close <= 1, the interval the moving placements of the scene file
    // ("transform_close") are sampled over; absent: [0, 1].  A bad value throws an error that names the key; so does the
    // key on a scene where nothing moves (the caller's check: it knows the scene).
    bool hasShutter() const { return !m_json["shutter"].isNull(); }
    void shutter(float *open, float *close) const;
    int gpu() const { return m_json["gpu"].isNumber() ? m_json["gpu"].asInt() : 0; }
    std::string assetRoot() const { return m_json["asset_root"].isString() ? m_json["asset_root"].asString() : ""; }
    std::string bvhBuilder() const { return m_json["bvh_builder"].isString() ? m_json["bvh_builder"].asString() : "auto"; }
    // fan-in of several devices' sums: "rccl" (ONE ncclReduce; on distinct devices a missing RCCL is an ERROR, raised before the
    // scene is loaded; only replicas that share a device use peer copies instead) | "peer-copy" (hipMemcpyPeer + add, on request)
    std::string reduceMethod() const { return m_json["reduce"].isString() ? m_json["reduce"].asString() : "rccl"; }
    // metrics.json: "full" (default) adds rays per sample, Mrays/s, algorithmic bytes and the roofline fraction from a
    // one-sample counting pass after the render; "basic" leaves them out
    std::string metricsLevel() const { return m_json["metrics"].isString() ? m_json["metrics"].asString() : "full"; }

    // string -> class factory, src/job.cpp:65-97; only the hot-path integrators exist here
    std::shared_ptr<Integrator> integrator() const;

    const Json &json() const { return m_json; }

private:
    Json m_json;
    BounceController m_bounceController;
};

}  // namespace pathed
