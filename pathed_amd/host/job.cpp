#include "job.h"

#include "integrator.h"

#include <cerrno>
#include <fstream>
#include <iostream>
#include <sys/stat.h>

namespace pathed {

Job::Job(const std::string &jobPath)
    : Job(Json::parseFile(jobPath))
{}

Job::Job(const Json &json)
    : m_json(json),
      m_bounceController(json["startBounce"].asInt(), json["lastBounce"].asInt())
{}

void Job::init()
{
    const std::string directory = outputDirectory();

    const int result = mkdir(directory.c_str(), S_IRWXU | S_IRWXG | S_IROTH | S_IXOTH);
    if (result == -1) {
        if (errno == EEXIST) {
            std::cout << "Output directory already exists: " << directory << std::endl;
        } else {
            std::cout << "Failed to create: " << directory << std::endl;
        }
        if (!force()) { throw std::runtime_error("output directory exists and \"force\" is not set"); }
    }

    std::ofstream report(directory + "/report.json");
    report << m_json.dump(4) << std::endl;
}

unsigned long long Job::seed() const
{
    const Json &seed = m_json["seed"];
    if (!m_json.has("seed")) { return 1ull; }
    if (!seed.isUnsigned()) { throw std::runtime_error("job: \"seed\" must be an integer in [0, 2^64), written in plain digits"); }
    return (unsigned long long)seed.asUnsigned();
}

std::vector<int> Job::devices() const
{
    const Json &gpus = m_json["gpus"];
    std::vector<int> ids;
    if (gpus.isArray()) {
        for (size_t i = 0; i < gpus.size(); i++) { ids.push_back(gpus[i].asInt()); }
    } else {
        const int count = gpus.isNumber() ? gpus.asInt() : 1;
        for (int i = 0; i < count; i++) { ids.push_back(gpu() + i); }
    }
    if (ids.empty() || ids.size() > 64) { throw std::runtime_error("job: \"gpus\" must name 1..64 devices"); }
    for (int id : ids) { if (id < 0) { throw std::runtime_error("job: negative device id in \"gpus\""); } }
    return ids;
}

std::vector<std::string> Job::features() const
{
    const Json &wanted = m_json["features"];
    std::vector<std::string> names;
    if (wanted.isNull()) { return names; }
    if (!wanted.isArray()) { throw std::runtime_error("job: \"features\" must be a list of names out of albedo, normal, depth"); }
    bool want[3] = { false, false, false };
    static const char *known[3] = { "albedo", "normal", "depth" };
    for (size_t i = 0; i < wanted.size(); i++) {
        if (!wanted[i].isString()) { throw std::runtime_error("job: \"features\" must be a list of names out of albedo, normal, depth"); }
        const std::string &name = wanted[i].asString();
        bool found = false;
        for (int k = 0; k < 3; k++) { if (name == known[k]) { want[k] = true; found = true; } }
        if (!found) { throw std::runtime_error("job: unknown feature \"" + name + "\" (known: albedo, normal, depth)"); }
    }
    for (int k = 0; k < 3; k++) { if (want[k]) { names.push_back(known[k]); } }
    return names;
}

void Job::shutter(float *open, float *close) const
{
    *open = 0.f;
    *close = 1.f;
    const Json &value = m_json["shutter"];
    if (value.isNull()) { return; }
    const char *rule = "job: \"shutter\" must be [open, close] with 0 <= open <= close <= 1";
    if (!value.isArray() || value.elements().size() != 2 || !value.elements()[0].isNumber() || !value.elements()[1].isNumber()) { throw std::runtime_error(rule); }
    const float first = (float)value.elements()[0].asNumber(), last = (float)value.elements()[1].asNumber();
    if (!(0.f <= first && first <= last && last <= 1.f)) { throw std::runtime_error(rule); }
    *open = first;
    *close = last;
}

Job::NoiseSettings Job::noise() const
{
    NoiseSettings settings;
    const Json &target = m_json["target_noise"];
    if (!target.isNull()) {
        if (!target.isNumber() || !(target.asNumber() > 0.0) || !(target.asNumber() < 1e30)) { throw std::runtime_error("job: \"target_noise\" must be a number > 0"); }
        settings.target = target.asNumber();
    }
    const Json &minSpp = m_json["min_spp"];
    if (!minSpp.isNull()) {
        if (!minSpp.isNumber() || minSpp.asNumber() != (double)(long long)minSpp.asNumber() || minSpp.asNumber() < 2.0 || minSpp.asNumber() > 1e9) {
            throw std::runtime_error("job: \"min_spp\" must be an integer >= 2");
        }
        settings.minSpp = (int)minSpp.asNumber();
    }
    const Json &floor = m_json["noise_floor"];
    if (!floor.isNull()) {
        if (!floor.isNumber() || !(floor.asNumber() > 0.0) || !(floor.asNumber() < 1e30)) { throw std::runtime_error("job: \"noise_floor\" must be a number > 0"); }
        settings.floor = floor.asNumber();
    }
    const Json &image = m_json["stderr_image"];
    if (!image.isNull() && !image.isBool()) { throw std::runtime_error("job: \"stderr_image\" must be true or false"); }
    settings.collect = settings.target > 0.0 || (image.isBool() && image.asBool());
    const Json &adaptive = m_json["adaptive"];
    if (!adaptive.isNull() && !adaptive.isBool()) { throw std::runtime_error("job: \"adaptive\" must be true or false"); }
    settings.adaptive = adaptive.isBool() && adaptive.asBool();
    if (settings.adaptive) {
        if (!(settings.target > 0.0)) { throw std::runtime_error("job: \"adaptive\" needs \"target_noise\": the pixels above it are the ones rendered on"); }
        if (resume()) { throw std::runtime_error("job: \"adaptive\" does not go with \"resume\": the state file holds neither squares nor counts"); }
        if (devices().size() != 1) { throw std::runtime_error("job: \"adaptive\" renders on one GPU: \"gpus\" must be 1 (a pixel list is not sharded)"); }
        if (integratorName() == "AlbedoIntegrator") { throw std::runtime_error("job: \"adaptive\" does not go with the AlbedoIntegrator, which keeps no second moments"); }
    }
    if (settings.collect && resume()) {
        throw std::runtime_error(std::string("job: \"resume\" does not go with \"") + (settings.target > 0.0 ? "target_noise" : "stderr_image")
                                 + "\": the state file holds no squares");
    }
    if (settings.collect && integratorName() == "AlbedoIntegrator") {
        throw std::runtime_error(std::string("job: \"") + (settings.target > 0.0 ? "target_noise" : "stderr_image") + "\" does not go with the AlbedoIntegrator, which keeps no second moments");
    }
    return settings;
}

std::shared_ptr<Integrator> Job::integrator() const
{
    const std::string name = integratorName();
    if (name == "PathTracer") {
        return std::make_shared<HipPathTracer>(m_bounceController);
    } else if (name == "VolumePathTracer") {
        // src/job.cpp:71-72: participating media behind passthrough containers
        return std::make_shared<HipPathTracer>(m_bounceController, PATHED_INTEGRATOR_VOLUME_PATH_TRACER);
    } else if (name == "BasicVolumeIntegrator") {
        // src/job.cpp:73-74: multiple scattering, a stack of media
        return std::make_shared<HipPathTracer>(m_bounceController, PATHED_INTEGRATOR_BASIC_VOLUME);
    } else if (name == "AlbedoIntegrator") {
        // src/job.cpp:91: a SampleIntegrator whose L is material->albedo(intersection)
        return std::make_shared<HipPathTracer>(m_bounceController, PATHED_INTEGRATOR_ALBEDO);
    } else if (name == "DataParallelIntegrator") {
        // the reference's stage-wise integrator needs its external sampler server; its
        // wavefront STRUCTURE is what HipPathTracer implements
        return std::make_shared<HipPathTracer>(m_bounceController);
    }
    throw std::runtime_error("Unimplemented");  // the reference throws "Unimplemented" (src/job.cpp:96)
}

}  // namespace pathed
