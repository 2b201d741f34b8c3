"""The anisotropic kernels (kernels.h: k_path_aniso, k_path_aniso_grid) in the code object of the built library: exactly four
exist, none takes more than 128 registers (four waves per SIMD, as the other volume kernels), and none needs more scratch than
DESIGN.md §4.4g states.  Read from the library's metadata, as tests/test_grid_kernel_resources.py does."""
from test_grid_kernel_resources import kernel_metadata

ANISO_KERNELS = {   # <STACK, SMALL>: scratch bytes per lane, as in DESIGN.md §4.4g
    "12k_path_anisoILi8ELb1EE": 296,
    "12k_path_anisoILi22ELb0EE": 412,
    "17k_path_aniso_gridILi8ELb1EE": 580,
    "17k_path_aniso_gridILi22ELb0EE": 576,
}


def test_anisotropic_instantiations_and_their_resources(tmp_path):
    kernels = kernel_metadata(tmp_path)
    aniso = {name: usage for name, usage in kernels.items() if "k_path_aniso" in name}
    print(aniso)
    assert len(aniso) == 4, sorted(aniso)
    for tag, scratch in ANISO_KERNELS.items():
        found = [usage for name, usage in aniso.items() if tag in name]
        assert len(found) == 1, (tag, found)
        registers, bytes_per_lane = found[0]
        assert registers <= 128 and bytes_per_lane <= scratch, (tag, found[0])
    # their names keep them out of the counts the other resource tests take by substring
    assert not [name for name in aniso if "k_path_scatter" in name or "k_path_volume" in name or "k_list_volume" in name]
    assert any("16k_debug_phase_hg" in name for name in kernels)
