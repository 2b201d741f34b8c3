"""The record arrays of tests/shading_cases.py through the CPU oracle alone: every edge the generator claims to contain is
there, and the branch it is meant to reach is taken (seen in the zero, infinite, not-a-number and swapped results the branch
produces).  tests/test_gpu_shading_queries.py feeds the same arrays to the device."""
import numpy as np
import pytest

import oracle_lib
import shading_cases as sc

F32 = np.float32


def rows(labels, *words):
    return np.array([all(word in label for word in words) for label in labels])


@pytest.fixture(scope="module")
def f_results():
    records, labels = sc.material_f_cases()
    return records, labels, sc.oracle_rows("material_f", records, 4)


@pytest.fixture(scope="module")
def sample_results():
    records, labels = sc.material_sample_cases()
    return records, labels, sc.oracle_rows("material_sample", records, 7)


def test_groups_are_small_and_deterministic():
    for records in (sc.material_f_cases()[0], sc.material_sample_cases()[0], sc.fresnel_cases(), sc.sphere_cases()[0]):
        assert 0 < len(records) <= 8192
    sc.material_f_cases.cache_clear()
    again = sc.material_f_cases()[0]
    assert again.tobytes() == sc.material_f_cases()[0].tobytes()
    for name in sc.environment_maps():
        assert 0 < len(sc.env_sample_cases(name)) <= 8192 and 0 < len(sc.env_direction_cases(name)[0]) <= 8192


def test_every_traits_set_accepts_some_records_and_all_accepts_every_one():
    records = sc.material_f_cases()[0]
    assert sc.accepts("All", records).all()
    for traits in sc.TRAITS:
        assert sc.accepts(traits, records).any()
    assert not sc.accepts("RoughBeckmann", records)[records[:, 19] == sc.GGX][records[records[:, 19] == sc.GGX][:, 0] == sc.MICROFACET].any()


def test_material_f_directions_reach_their_branches(f_results):
    records, labels, out = f_results
    kind = records[:, 0].astype(int)
    f, pdf = out[:, :3], out[:, 3]
    # the degenerate frame: wo exactly the normal
    assert (records[:, 23:26] == records[:, 26:29]).all(axis=1).any()
    # wo below the surface: Lambertian and microfacet black with pdf 0, Oren-Nayar with its pdf of 1
    under = rows(labels, "wo below the surface")
    for k in (sc.LAMBERTIAN, sc.MICROFACET, sc.PLASTIC):
        assert (f[under & (kind == k)] == 0).all() and (pdf[under & (kind == k)] == 0).all()
    assert (f[under & (kind == sc.OREN_NAYAR)] == 0).all() and (pdf[under & (kind == sc.OREN_NAYAR)] == 1).all()
    # ... also where only the tilted shading normal says so
    tilted = rows(labels, "below the tilted shading normal only")
    assert (pdf[tilted & (kind == sc.LAMBERTIAN)] == 0).all()
    # wi below the horizon
    horizon = rows(labels, "cos 0.7", "below the horizon")
    assert (pdf[horizon & (kind == sc.LAMBERTIAN)] == 0).all() and (pdf[horizon & (kind == sc.OREN_NAYAR)] == 1).all()
    # wh at the pole (the mirror direction): the largest D there is; for Beckmann at alpha 1e-3 that is 1 / (pi alpha^2)
    mirror = rows(labels, "microfacet beckmann alpha 0.001", "cos 0.7", "mirror")
    assert mirror.sum() == 1 and pdf[mirror][0] > 1e4 and np.isfinite(out[mirror]).all()
    # wi = -wo: below the surface and black, unless wo lies IN the surface: then the zero half vector, normalised, is not a number
    opposite = rows(labels, "cos 0.7", "minus wo") & (kind == sc.MICROFACET)
    assert (pdf[opposite] == 0).all()
    opposite = rows(labels, "cos 0 |", "minus wo") & (kind == sc.MICROFACET)
    assert np.isnan(pdf[opposite]).all()
    # grazing wo: cos 0 ends in the early return, black
    level = rows(labels, "cos 0 |") & (kind == sc.MICROFACET)
    assert (f[level] == 0).all()
    # glass and mirror evaluate to nothing
    assert (out[(kind == sc.GLASS) | (kind == sc.MIRROR)] == 0).all()
    # exact zeros and NaNs both occur, so their POSITIONS are a real check on the device
    assert (out == 0).any() and np.isnan(out).any()


def test_material_f_has_components_on_either_side_of_the_clamp():
    """TangentFrame::clamp replaces a vector by an axis when a component reaches 0.9999 -- in sinPhi alone"""
    for label, normal, shading, wo in sc.surfaces():
        if "cos 0.7" not in label:
            continue
        local_wo = sc.to_local(shading, wo, wo)
        found = {}
        for wlabel, wi in sc.incident_directions(normal, shading, wo):
            local_wi = sc.to_local(shading, wo, wi)
            if wlabel.startswith("wi."):
                axis = "xyz".index(wlabel[3])
                found.setdefault(("wi", axis, bool(abs(local_wi[axis]) >= sc.CLAMP)), wlabel)
            if wlabel.startswith("wh."):
                axis = "xyz".index(wlabel[3])
                wh = (local_wo + local_wi) / np.linalg.norm(local_wo + local_wi)
                found.setdefault(("wh", axis, bool(abs(wh[axis]) >= sc.CLAMP)), wlabel)
        for which in ("wi", "wh"):
            for axis in range(3):
                assert (which, axis, True) in found and (which, axis, False) in found, (which, axis, found)


def test_checkerboard_cells(f_results):
    records, labels, out = f_results
    board = rows(labels, "checkerboard", "cos 0.7") & (out[:, 3] > 0)
    on, off = F32(0.9) / F32(np.pi), F32(0.1) / F32(np.pi)
    assert np.isclose(out[board, 0], on, rtol=1e-6).any() and np.isclose(out[board, 0], off, rtol=1e-6).any()
    assert (records[board, 29] < 0).any()                                  # negative uv
    assert (records[board, 29] * 4 == np.floor(records[board, 29] * 4)).any()    # uv on a cell border


def test_plastic_takes_the_lambertian_lobe_above_one_half_only(sample_results):
    records, labels, out = sample_results
    for dist in ("beckmann", "ggx"):
        chosen = rows(labels, "plastic %s alpha 0.3" % dist, "cos 0.7")
        by_script = {tuple(records[i, 31:34]): out[i, :3] for i in np.flatnonzero(chosen)}
        lower, half, upper = (F32(u) for u in sc.U_HALF)
        pair = (F32(0.83), F32(0.29))
        assert np.array_equal(by_script[(lower,) + pair], by_script[(half,) + pair])
        assert not np.array_equal(by_script[(upper,) + pair], by_script[(half,) + pair])
        # the Lambertian lobe's direction does not depend on alpha: the same under every alpha
        other = rows(labels, "plastic %s alpha 0.05" % dist, "cos 0.7")
        by_script_other = {tuple(records[i, 31:34]): out[i, :3] for i in np.flatnonzero(other)}
        assert np.array_equal(by_script[(upper,) + pair], by_script_other[(upper,) + pair])
        assert not np.array_equal(by_script[(half,) + pair], by_script_other[(half,) + pair])


def test_glass_reflects_below_the_reflectance_only_and_swaps_inside(sample_results):
    records, labels, out = sample_results
    chosen = np.flatnonzero(rows(labels, "glass ior 1.4", "cos 0.7"))
    reflectance = sc.fresnel_of(float(F32(0.7)), 1.0, float(F32(1.4)))
    below, at, above = (F32(u) for u in sc.around(reflectance))
    side = {records[i, 31]: out[i, 1] for i in chosen}     # y of wi: up = reflected (the normal is +y, wo above)
    assert side[below] > 0 and side[at] < 0 and side[above] < 0
    pdf = {records[i, 31]: out[i, 3] for i in chosen}
    assert pdf[below] == F32(reflectance) and pdf[at] == F32(1) - F32(reflectance)
    # from inside, the etas swap: the refracted ray leaves upwards and bends AWAY from the normal
    inside = np.flatnonzero(rows(labels, "glass ior 1.4", "wo below the surface"))
    refracted = [i for i in inside if out[i, 1] > 0]
    assert refracted and all(abs(out[i, 0]) > abs(records[i, 26]) for i in refracted)
    # around the critical angle: total reflection (pdf 1 whatever u) on one side, refraction on the other
    critical = np.flatnonzero(rows(labels, "glass ior 2.4", "inside, cos"))
    assert (out[critical, 3] == 1).any() and ((out[critical, 3] < 1) & (out[critical, 1] > 0)).any()
    # ior 1: nothing reflects
    assert (out[rows(labels, "glass ior 1 ", "cos 0.7"), 1] < 0).all()


def test_sampling_edges_of_the_distributions(sample_results):
    records, labels, out = sample_results
    wo = np.array(sc._with_cosine(F32(0.7)), dtype=F32)
    mirror = wo * np.array([-1, 1, -1], dtype=F32)
    # Beckmann: xi == 0 -> logf(0) = -inf -> replaced by 0 -> wh at the pole -> the mirror direction
    chosen = rows(labels, "microfacet beckmann alpha 0.3", "cos 0.7") & (records[:, 32] == 0)
    assert chosen.sum() >= 3 and np.abs(out[chosen, :3] - mirror).max() < 1e-6
    # GGX: xi1 = 1 - 2^-24 -> sqrtf(1 - xi1) = 2^-12 -> a half vector near the horizon
    assert oracle_lib.evaluate("ggx_sample", [1.0, sc.ALMOST_ONE, 0.37])[1] < 1e-3
    assert (rows(labels, "microfacet ggx") & (records[:, 31] == F32(sc.ALMOST_ONE))).any()
    # u = 0 and u = 1 - 2^-24 reach the cosine-hemisphere sampler: straight up, and the horizon
    up = rows(labels, "lambertian", "cos 0.7") & (records[:, 31] == 0)
    assert np.allclose(out[up, :3], (0, 1, 0), atol=1e-6)
    flat = rows(labels, "lambertian", "cos 0.7") & (records[:, 31] == F32(sc.ALMOST_ONE))
    assert (np.abs(out[flat, 1]) < 1e-3).all()
    assert (out == 0).any() and np.isnan(out).any()


def test_fresnel_cases_reach_total_reflection_and_both_orders():
    records = sc.fresnel_cases()
    out = sc.oracle_rows("fresnel", records, 1)[:, 0]
    assert (out == 1).any() and (out == 0).any() and ((out > 0) & (out < 1)).any()
    for ior in (1.4, 2.4):
        cosines = sc.critical_cosines(ior)
        values = [sc.fresnel_of(c, float(F32(ior)), 1.0) for c in cosines]
        assert values[0] == 1.0 and values[-1] < 1.0


def test_sphere_cases_reach_both_measures_and_the_cancellation():
    samples, pdfs, labels = sc.sphere_cases()
    out = sc.oracle_rows("sphere_sample", samples, 8)
    inside = rows(labels, "inside")
    assert (out[inside, 7] == 1).all()           # area measure
    far = rows(labels, "1e4 r")
    assert (out[far, 7] == 0).all()
    assert (out[far, 6] == 0).all()              # 1 - cosThetaMax cancelled: an infinite pdf, a zero inverse
    near = rows(labels, "1.15 r")
    assert (out[near, 7] == 0).all() and (out[near, 6] > 0).all()
    # the sampled point lies on the sphere
    distance = np.linalg.norm(out[:, :3].astype(np.float64) - np.asarray(sc.SPHERE_CENTRE), axis=1)
    assert np.abs(distance[np.isfinite(distance)] - sc.SPHERE_RADIUS).max() < 1e-5
    assert np.isfinite(sc.oracle_rows("sphere_pdf", pdfs, 1)).sum() >= len(pdfs) - 4 * 1


@pytest.mark.parametrize("name", sorted(sc.environment_maps()))
def test_environment_samples_against_the_linear_scan_and_the_record_model(name):
    """the oracle's steps are the linear scan's over the CDFs as restated in numpy; the numpy model of the device's per-cell
    records chooses the same index and pdf in every case"""
    theta, theta_empty, phis, phi_empty = sc.environment_cdfs(name)
    records = sc.env_sample_cases(name)
    out = sc.oracle_env_rows(name, "env_sample_steps", records, 9)
    paths = set()
    for record, result in zip(records, out):
        row, row_pdf = sc.linear_scan(theta, theta_empty, record[3])
        column, column_pdf = sc.linear_scan(phis[row], phi_empty[row], record[4])
        assert (result[7], result[8]) == (row, column), (record, result)
        model_row = sc.record_sample(theta, theta_empty, record[3])
        model_column = sc.record_sample(phis[row], phi_empty[row], record[4])
        assert model_row[:2] == (row, row_pdf) and model_column[:2] == (column, column_pdf), (record, model_row, model_column)
        paths.update(("theta " + model_row[2], "phi " + model_column[2]))
    print(name, sorted(paths))
    if name == "sparse 64x33":
        assert {"phi rare", "phi lo", "phi lo + 1", "phi lo + 2", "phi empty", "theta lo"} <= paths
        # xi == 0 picks the black row 0: an infinite inverse pdf
        first = (records[:, 3] == 0)
        assert (out[first, 7] == 0).all() and np.isinf(out[first, 6]).all()
    if name == "black 5x3":
        assert paths == {"theta empty", "phi empty"} and np.isinf(out[:, 6]).all()


@pytest.mark.parametrize("name", sorted(sc.environment_maps()))
def test_environment_directions_land_in_their_texels(name):
    directions, texels = sc.env_direction_cases(name)
    parts = sc.oracle_env_rows(name, "env_pdf_parts", directions, 4)
    assert np.array_equal(parts[:, 1:3].astype(int), texels)
    rgba, scale, _ = sc.environment_maps()[name]
    emitted = sc.oracle_env_rows(name, "env_emit", -directions, 3)
    expected = rgba[texels[:, 0], texels[:, 1], :3] * F32(scale)
    assert np.array_equal(emitted, expected)


FURNACE_LABELS = [entry[0] for entry in sc.furnace_cases()]


def test_furnace_cases_are_the_issues_and_tight_enough():
    assert len(FURNACE_LABELS) == 24
    for label in FURNACE_LABELS:
        expected = sc.furnace_expectation(label)[0]
        assert sc.furnace_allowance(label, 2 ** 16) <= 0.03 * expected, label


@pytest.mark.parametrize("label", FURNACE_LABELS)
def test_furnace_on_the_oracle(label):
    """the oracle's material_sample, 2^12 stratified scripted samples, against the float64 quadrature of f cos: what
    tests/test_gpu_shading_queries.py asks of the device at 2^16"""
    entry = next(e for e in sc.furnace_cases() if e[0] == label)
    side = 64
    estimate = sc.furnace_estimate(sc.oracle_rows("material_sample", sc.furnace_records(entry, side), 7))
    expected = sc.furnace_expectation(label)[0]
    allowance = sc.furnace_allowance(label, side * side)
    print("%-40s expected %.6f estimate %.6f difference %.2e allowance %.2e" % (label, expected, estimate, abs(estimate - expected), allowance))
    assert abs(estimate - expected) <= allowance
