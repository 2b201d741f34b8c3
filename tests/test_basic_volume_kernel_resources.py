"""The BasicVolumeIntegrator's kernels (kernels.h: k_path_scatter, k_path_scatter_grid) in the code object of the built library:
exactly eight exist, none takes more than 128 registers (four waves per SIMD, as the other volume kernels), and none needs more
scratch than DESIGN.md §4.4f states.  Read from the library's metadata, as tests/test_grid_kernel_resources.py does."""
from test_grid_kernel_resources import kernel_metadata

SCATTER_KERNELS = {   # <STACK, SMALL>: scratch bytes per lane, as in DESIGN.md §4.4f
    "14k_path_scatterILi8ELb1EE": 220,
    "14k_path_scatterILi8ELb0EE": 364,
    "14k_path_scatterILi16ELb0EE": 364,
    "14k_path_scatterILi22ELb0EE": 364,
    "19k_path_scatter_gridILi8ELb1EE": 612,
    "19k_path_scatter_gridILi8ELb0EE": 600,
    "19k_path_scatter_gridILi16ELb0EE": 600,
    "19k_path_scatter_gridILi22ELb0EE": 600,
}


def test_scatter_instantiations_and_their_resources(tmp_path):
    kernels = kernel_metadata(tmp_path)
    scatter = {name: usage for name, usage in kernels.items() if "k_path_scatter" in name}
    print(scatter)
    assert len(scatter) == 8, sorted(scatter)
    for tag, scratch in SCATTER_KERNELS.items():
        found = [usage for name, usage in scatter.items() if tag in name]
        assert len(found) == 1, (tag, found)
        registers, bytes_per_lane = found[0]
        assert registers <= 128 and bytes_per_lane <= scratch, (tag, found[0])
    assert any("21k_debug_phase_samples" in name for name in kernels)
