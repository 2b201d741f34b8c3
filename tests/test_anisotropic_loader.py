"""The scene file's "phase" key (pathed_amd/host/scene_loader.cpp: parsePhase): a medium of either kind may carry
{"type": "henyey-greenstein", "g": "0.8"}; it reaches FlatScene::phases and LoadedScene.phases as (medium slot, g); "isotropic"
and no key leave no entry; any other type is refused by name."""
import json

import numpy as np
import pytest

from pathed_amd.scene import LoadedScene

SCENE = {
    "sensor": {"lookAt": {"origin": ["0", "1", "6"], "target": ["0", "1", "0"], "up": ["0", "1", "0"]}, "fov": "20"},
    "media": [
        {"name": "plain", "type": "homogeneous", "sigma_t": ["1", "1", "1"], "sigma_s": ["1", "1", "1"]},
        {"name": "forward", "type": "homogeneous", "sigma_t": ["2", "2", "2"], "sigma_s": ["1", "1", "1"],
         "phase": {"type": "henyey-greenstein", "g": "0.8"}},
        {"name": "named", "type": "homogeneous", "sigma_t": ["1", "1", "1"], "sigma_s": ["1", "1", "1"], "phase": {"type": "isotropic"}},
        {"name": "backward", "type": "homogeneous", "sigma_t": ["1", "1", "1"], "sigma_s": ["1", "1", "1"],
         "phase": {"type": "henyey-greenstein", "g": "-0.35"}},
    ],
    "models": [],
}


def _load(tmp_path, scene):
    (tmp_path / "scene.json").write_text(json.dumps(scene))
    return LoadedScene("scene.json", 16, 12, asset_root=str(tmp_path))


def test_the_phase_key_reaches_the_flat_scene(tmp_path):
    scene = _load(tmp_path, SCENE)
    assert scene.desc.contents.n_media == 4
    assert scene.phases == [(1, float(np.float32(0.8))), (3, float(np.float32(-0.35)))]
    assert _load(tmp_path, {**SCENE, "media": SCENE["media"][:1]}).phases == []


def test_an_unknown_phase_function_is_refused_by_name(tmp_path):
    broken = json.loads(json.dumps(SCENE))
    broken["media"][1]["phase"]["type"] = "rayleigh"
    with pytest.raises(RuntimeError, match="rayleigh"):
        _load(tmp_path, broken)


@pytest.mark.parametrize("g, message", [("1.0", "0.99"), ("-0.995", "0.99"), ("nan", "0.99"), (None, '"g"')])
def test_a_bad_mean_cosine_is_refused(tmp_path, g, message):
    broken = json.loads(json.dumps(SCENE))
    if g is None:
        del broken["media"][1]["phase"]["g"]
    else:
        broken["media"][1]["phase"]["g"] = g
    with pytest.raises(RuntimeError) as error:
        _load(tmp_path, broken)
    assert message in str(error.value), str(error.value)


def test_the_binding_mirrors_the_header(tmp_path):
    """PathedPhaseFunction's size, the type codes and the threshold as the C compiler sees include/pathed_hip.h"""
    import ctypes as C
    import os
    import subprocess
    from pathed_amd import _capi
    (tmp_path / "phase.c").write_text(
        '#include "pathed_hip.h"\n#include <stdio.h>\n'
        'int main(void){printf("%zu %d %d %.17g\\n", sizeof(PathedPhaseFunction), PATHED_PHASE_ISOTROPIC, PATHED_PHASE_HENYEY_GREENSTEIN,'
        ' (double)PATHED_PHASE_ISOTROPIC_BELOW);return 0;}\n')
    exe = str(tmp_path / "phase")
    subprocess.run(["gcc", "-I", os.path.join(_capi.REPO_ROOT, "include"), str(tmp_path / "phase.c"), "-o", exe], check=True)
    size, isotropic, henyey, below = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == C.sizeof(_capi.PathedPhaseFunction) == 12
    assert (int(isotropic), int(henyey)) == (_capi.PHASE_ISOTROPIC, _capi.PHASE_HENYEY_GREENSTEIN)
    assert float(below) == _capi.PHASE_ISOTROPIC_BELOW


def test_the_shipped_plume_scene_carries_its_phase_function():
    """scenes/cornell-smoke-hg.json: the plume of scenes/cornell-smoke.json at g = 0.8, on the grid's slot"""
    scene = LoadedScene("scenes/cornell-smoke-hg.json", 32, 32)
    assert [slot for slot, _ in scene.grids] == [0]
    assert scene.phases == [(0, float(np.float32(0.8)))]
    assert LoadedScene("scenes/cornell-smoke.json", 32, 32).phases == []
