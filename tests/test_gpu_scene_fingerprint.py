"""What scene creation leaves on the device, pinned: tools/scene_fingerprint.py hashes, per scene, the tree, the light records,
the item order, the camera masks, the placements' records, the statistics that name the kernel choice and a small render; the
hashes recorded on the commit named in tests/golden/scene_fingerprints.json must come out again, section by section, so that a
change of the host code that builds a scene names the table it moved.  Refused creations are pinned by code and message.
And a refused creation leaves nothing behind on the device."""
import importlib.util
import json
import os

import pytest

from pathed_amd import _capi

pytestmark = pytest.mark.gpu


def _tool():
    spec = importlib.util.spec_from_file_location("scene_fingerprint", os.path.join(_capi.REPO_ROOT, "tools", "scene_fingerprint.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


TOOL = _tool()
with open(os.path.join(_capi.REPO_ROOT, "tests", "golden", "scene_fingerprints.json")) as handle:
    GOLDEN = json.load(handle)


def test_the_recorded_scenes_are_the_tools():
    assert list(GOLDEN["scenes"]) == list(TOOL.SCENES) and GOLDEN["recorded_on"]


@pytest.mark.parametrize("name", list(TOOL.SCENES))
def test_scene_creation_leaves_the_recorded_tables(name):
    expected = GOLDEN["scenes"][name]
    found = TOOL.fingerprint(name)
    print(name, json.dumps(found))
    for section in expected:
        assert found.get(section) == expected[section], (name, section)
    assert set(found) == set(expected)
    if "render_after_refit" in found:   # a refit with the positions the scene was created with moves nothing
        assert found["render_after_refit"] == found["render"]


def _pages(n_bytes, page=4096):
    return (n_bytes + page - 1) // page * page


def test_a_refused_creation_leaves_nothing_on_the_device():
    """shade_kernel = fused on the few-hundred-triangle mesh is refused after the tree and the tables are uploaded (the soup is
    gone by then).  One such scene's footprint, from the sizes of the buffers it holds at that point (pathed_hip.hip:
    uploadTextures, uploadSoup, buildTreeOnHost, uploadShadingTables), each rounded up to a 4 KiB page; 50 refusals may cost
    no more than that (the allocator may keep a block: equality is not asked).  Measured: 0 bytes against a footprint of
    139 264.  (Run alone the test takes 11 s, torch's start-up; in the suite, where torch is up already, under 3.5 s.)"""
    import torch
    from pathed_amd.integrator import HipScene, PathedError
    built, desc = TOOL.mesh_scene()
    d = desc.contents
    good = HipScene(desc, device=0)
    n_nodes = int(good.stats()["bvh_nodes"])
    good.close()
    nt, ns, n_lights = int(d.n_triangles), int(d.n_spheres), 1     # the environment is the one light
    w, h = int(d.env.contents.width), int(d.env.contents.height)
    texels = sum(int(d.textures[t].width) * int(d.textures[t].height) for t in range(int(d.n_textures)))
    buffers = [16 * texels, 128 * nt, 32 * nt,                      # texels, triShade, triCompact
               128 * n_nodes, 48 * nt,                              # nodes, leaf triangles
               32 * ns, 96 * int(d.n_materials), 8 * n_lights, 64 * n_lights, 32 * int(d.n_media), 4 * (nt + ns),
               16 * w * h, 4 * h, 4 * w * h, 4 * h, 4 * (h + 1), 4 * h * (w + 1), 32 * (h + 1), 32 * h * (w + 1)]   # the environment's tables
    footprint = sum(_pages(size) for size in buffers if size)

    def refuse():
        with pytest.raises(PathedError, match="the fused path kernel serves scenes of at most 64 triangles"):
            HipScene(desc, device=0, shade_kernel="fused", build_threads=1)     # (one builder thread: the tree does not depend on it)

    refuse()                                     # (whatever the first refusal sets up once is not counted)
    torch.cuda.synchronize(0)
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):
        refuse()
    torch.cuda.synchronize(0)
    after = torch.cuda.mem_get_info(0)[0]
    print("free before %d after %d: fell by %d bytes; one scene's footprint %d bytes" % (before, after, before - after, footprint))
    assert before - after <= footprint
