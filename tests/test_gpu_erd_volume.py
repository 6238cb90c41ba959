"""-m gpu: whole-volume AutoERD with the ERD-weighted direction means and ADC maps (erd.erd_volume, csrc/erd_volume.hip; david.py:44-91)
against the sklearn fixtures, the NumPy oracle, the existing per-slice kernel and the float64 restatement of
tests/erd_volume_common.py; the david driver and entry script on a synthetic patient.

Comparisons: acceptance weights and the four mean maps are array-equal to the restatement (NaN positions equal, finite values
bitwise equal).  ADC values are compared in float64 ULPs against V.ADC_ULP = 4 (erd_volume_common: 1 for each library's log + 2
for the roundings of / b and * 1000); every test prints the maximum it measured."""
import json

import numpy as np
import pytest

from oracle import erd_oracle as E
from tests import erd_volume_common as V

B = 900


def _check_against_restatement(got, want, label):
    assert np.array_equal(np.asarray(got.accept, np.float64), np.asarray(want.accept, np.float64)), label
    assert V.same_bits(got.direction_mean, want.direction_mean), label
    assert V.same_bits(got.accepted_mean, want.accepted_mean), label
    worst = 0
    for name in ("direction_adc", "accepted_adc", "adc"):
        g, w = getattr(got, name), getattr(want, name)
        if g is None:
            continue
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (label, name)
        d = V.max_ulp(g, w)
        print(f"{label} {name}: max ULP distance {d} (allowed {V.ADC_ULP})")
        assert d <= V.ADC_ULP, (label, name, d)
        worst = max(worst, d)
    return worst


@pytest.mark.gpu
def test_partitions_equal_the_sklearn_fixture(golden):
    """Every fixture sample as one pixel (grouped by length), rules 1 and 2: the expectations of
    test_erd.py::test_device_partitions_equal_sklearn_fixture, from sklearn's stored labels."""
    from mri_super_resolution_amd import erd
    g = golden("erd.npz")
    by_n = {}
    for v, n, lab in zip(g["values"], g["lengths"], g["labels"]):
        by_n.setdefault(int(n), []).append((v[:n], lab[:n]))
    checked = 0
    for n, items in by_n.items():
        img = np.stack([x for x, _ in items])
        for rule in (1, 2):
            got = erd.auto_erd_volume(img, rule)
            assert got.dtype == np.int64 and got.shape == img.shape
            for (x, lab), keep in zip(items, got):
                groups = (lab == 0, lab == 1)
                want = np.ones(n, np.int64)
                if rule == 1:
                    for k in range(2):
                        if groups[k].sum() >= (2 / 3) * n:
                            want[groups[1 - k]] = 0
                else:
                    means = [x[q].mean() for q in groups]
                    for k in range(2):
                        if means[k] > means[1 - k]:
                            want[groups[1 - k]] = 0
                assert np.array_equal(keep, want), (rule, x, lab, keep)
                checked += 1
    assert checked == 2 * 2460


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 31, 32])
def test_long_samples_and_ragged_pixel_counts(n):
    """Integer-valued samples with planted outliers, all-equal and two-valued pixels; 1, 63, 64, 65 and 1,025 pixels (one lane, a
    ragged wave, a full wave, one lane of a second block, many blocks).  Array-equal to the oracle and to the per-slice kernel."""
    from mri_super_resolution_amd import erd
    x = V.planted_samples(n, 1025, seed=100 + n)
    want1 = E.auto_erd(x[:, None, :], 1)[:, 0]
    want2 = E.auto_erd(x[:65, None, :], 2)[:, 0]
    assert (want1 == 0).any() and (want1.sum(-1) == n).any()
    for pixels in (1, 63, 64, 65, 1025):
        got = erd.auto_erd_volume(x[:pixels], 1)
        assert np.array_equal(got, want1[:pixels]), pixels
        assert np.array_equal(got, erd.auto_erd(x[:pixels].reshape(1, pixels, n), 1)[0]), pixels
    assert np.array_equal(erd.auto_erd_volume(x[:65], 2), want2)
    assert np.array_equal(erd.auto_erd_volume(x, 2), erd.auto_erd(x.reshape(1, 1025, n), 2)[0])
    assert np.array_equal(erd.auto_erd_volume(x.reshape(5, 41, 5, n), 1), want1.reshape(5, 41, 5, n))       # leading axes are free


@pytest.mark.gpu
def test_shortest_samples_and_limits():
    from mri_super_resolution_amd import erd
    rng = np.random.default_rng(3)
    two = np.round(rng.normal(100.0, 30.0, (70, 2)))
    assert erd.auto_erd_volume(two, 1).all()                                     # 1 + 1: no cluster reaches (2/3) * 2
    assert np.array_equal(erd.auto_erd_volume(two, 2), E.auto_erd(two[:, None, :], 2)[:, 0])
    three = np.full((3, 3), 7.0)
    got = erd.auto_erd_volume(three, 1)
    assert (got.sum(-1) == 2).all() and np.array_equal(got, E.auto_erd(three[:, None, :], 1)[:, 0])      # (2/3) * 3 == 2.0
    for n in (33, 1):
        with pytest.raises(Exception):
            erd.auto_erd_volume(np.zeros((4, n)), 1)
        with pytest.raises(Exception):
            erd.erd_volume(np.zeros((4, n)), np.ones(4), (n,), B)
    with pytest.raises(Exception):
        erd.auto_erd_volume(two, 3)
    with pytest.raises(Exception):
        erd.erd_volume(two, np.ones(70), (1, 2), B)                              # the groups do not sum to n
    with pytest.raises(Exception):
        erd.erd_volume(two, np.ones(70), (2,), 0)                                # b == 0
    with pytest.raises(Exception):
        erd.erd_volume(two, np.ones(70), (2,), B, rule=1, accept=np.ones((70, 2)))


@pytest.mark.gpu
def test_rule_2_rejects_only_where_the_erd_map_is_positive():
    from mri_super_resolution_amd import erd
    x = V.planted_samples(12, 70, seed=9).reshape(7, 10, 12)
    emap = np.tile(np.array([2.5, 0.0, -1.0, -np.inf, np.nan, 1e-300, np.inf], np.float64)[:, None], (1, 10))
    got = erd.auto_erd_volume(x, 2, emap)
    assert np.array_equal(got, V.accept_weights(x, 2, emap))
    assert got[1:5].all() and (got[0] == 0).any() and (got[5] == 0).any() and (got[6] == 0).any()
    assert np.array_equal(got[[0, 5, 6]], erd.auto_erd_volume(x, 2)[[0, 5, 6]])
    assert np.array_equal(erd.auto_erd_volume(x, 2, emap.astype(np.float32)), V.accept_weights(x, 2, emap.astype(np.float32)))


@pytest.mark.gpu
def test_non_finite_pixels_keep_every_acquisition():
    """Defined behaviour: a pixel with a NaN or an infinity among its acquisitions is not clustered (the kernel tests every value
    before it clusters and skips the walk) and keeps everything; the other pixels of its wave are clustered as if it were not
    there; its sums follow IEEE."""
    from mri_super_resolution_amd import erd
    clean, b0 = V.volume_case((70, 12), (4, 4, 4), seed=21)
    x = clean.copy()
    x[5, 3] = np.nan
    x[9, 0] = np.inf
    x[40, 11] = -np.inf
    x[66, 7] = np.nan                                                            # a lane of the second, ragged wave
    bad = [5, 9, 40, 66]
    for rule in (1, 2):
        got = erd.erd_volume(x, b0, (4, 4, 4), B, rule=rule, per_acquisition_adc=True)
        ref = erd.erd_volume(clean, b0, (4, 4, 4), B, rule=rule, per_acquisition_adc=True)
        assert got.accept[bad].all()
        good = np.setdiff1d(np.arange(70), bad)
        assert np.array_equal(got.accept[good], ref.accept[good])
        for name in ("direction_mean", "accepted_mean", "direction_adc", "accepted_adc"):
            assert V.same_bits(getattr(got, name)[:, good], getattr(ref, name)[:, good]), name
        _check_against_restatement(got, V.restate(x, b0, (4, 4, 4), B, rule=rule), f"non-finite rule {rule}")
        assert np.isnan(got.direction_mean[0, 5]) and got.direction_mean[0, 9] == np.inf and got.direction_mean[2, 40] == -np.inf
    # two finite values whose extent overflows: no neighbour is ever found, the pixel keeps both
    assert erd.auto_erd_volume(np.array([[1e308, -1e308], [3.0, 4.0]]), 2).tolist() == [[1, 1], [0, 1]]


CASES = [((5, 7, 3, 12), (4, 4, 4), None), ((9, 11, 1, 6), (1, 2, 3), 0), ((6, 5, 12), (12,), None)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,groups,dropout_group", CASES)
def test_means_and_adc_maps_against_the_restatement(shape, groups, dropout_group):
    from mri_super_resolution_amd import erd
    dwi, b0 = V.volume_case(shape, groups, seed=sum(shape), dropout_group=dropout_group)
    lead = shape[:-1]
    for rule in (1, 2):
        want = V.restate(dwi, b0, groups, B, rule=rule)
        got = erd.erd_volume(dwi, b0, groups, B, rule=rule, per_acquisition_adc=True)
        assert got.accept.shape == shape and got.accept.dtype == np.int64 and got.adc.shape == shape
        assert got.direction_mean.shape == (len(groups),) + lead == got.accepted_adc.shape
        _check_against_restatement(got, want, f"{shape} rule {rule}")
        assert erd.erd_volume(dwi, b0, groups, B, rule=rule).adc is None
    got = erd.erd_volume(dwi, b0, groups, B, rule=1, per_acquisition_adc=True)
    if dropout_group is not None:                                                 # the single-acquisition group is wholly rejected somewhere
        gone = np.isnan(got.accepted_mean[dropout_group])
        assert gone.any() and not gone.all() and np.array_equal(gone, got.accept[..., 0] == 0)
        assert np.array_equal(np.isnan(got.accepted_adc[dropout_group]), gone | np.isnan(got.direction_adc[dropout_group]))
    flat_adc, flat_mean = got.adc.reshape(-1, shape[-1]), got.direction_adc.reshape(len(groups), -1)
    assert np.isfinite(flat_adc[1]).all() and np.isfinite(flat_adc[2]).all()       # b0 == 0, with and without signal
    assert V.max_ulp([flat_adc[2, 0], flat_mean[0, 2]], [V.adc(0.0, 0.0, B)] * 2) <= V.ADC_ULP and flat_mean[0, 2] > 0      # -log(eps) / b
    assert np.isfinite(flat_adc[4, 0]) and np.isnan(flat_adc[6, -1])              # a zero acquisition; log of a negative number


@pytest.mark.gpu
def test_input_dtypes_and_device_tensors_give_the_same_results():
    import torch
    from mri_super_resolution_amd import erd
    dwi, b0 = V.volume_case((5, 7, 3, 12), (4, 4, 4), seed=27)
    dwi = np.clip(dwi, 0.0, None)                                                 # integer-valued and >= 0: exact in every dtype below
    ref = erd.erd_volume(dwi, b0, (4, 4, 4), B, rule=1, per_acquisition_adc=True)
    for dt in (np.float32, np.uint16):
        got = erd.erd_volume(dwi.astype(dt), b0.astype(dt), np.asarray([4, 4, 4]), B, rule=1, per_acquisition_adc=True)
        assert np.array_equal(got.accept, ref.accept) and got.accept.dtype == np.int64
        for name in ("direction_mean", "accepted_mean", "direction_adc", "accepted_adc", "adc"):
            assert V.same_bits(getattr(got, name), getattr(ref, name)), (dt, name)
    dev = erd.erd_volume(torch.from_numpy(dwi.astype(np.float32)).cuda(), torch.from_numpy(b0).cuda(), (4, 4, 4), B, rule=1,
                         per_acquisition_adc=True)
    for name in dev._fields:
        t = getattr(dev, name)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous(), name
        assert V.same_bits(t.cpu().numpy(), np.asarray(getattr(ref, name), np.float64)), name
    acc = erd.auto_erd_volume(torch.from_numpy(dwi).cuda(), 1)
    assert acc.is_cuda and np.array_equal(acc.cpu().numpy(), ref.accept)
    with pytest.raises(Exception):
        erd.erd_volume(torch.from_numpy(dwi), torch.from_numpy(b0), (4, 4, 4), B)      # host tensors: there is no CPU path


@pytest.mark.gpu
def test_rule_0_uses_supplied_weights_as_they_are():
    from mri_super_resolution_amd import erd
    dwi, b0 = V.volume_case((9, 11, 1, 6), (1, 2, 3), seed=5)
    dwi = dwi + 0.1                                                               # inexact products with the weights below
    rng = np.random.default_rng(12)
    w = rng.choice([0.0, 0.3, 0.7, 1.0, 1.0 / 3.0], dwi.shape)                    # v * w is inexact: a contracted multiply-add would show
    got = erd.erd_volume(dwi, b0, (1, 2, 3), B, rule=0, accept=w, per_acquisition_adc=True)
    assert got.accept.dtype == np.float64 and np.array_equal(got.accept, w)
    _check_against_restatement(got, V.restate(dwi, b0, (1, 2, 3), B, rule=0, accept=w), "rule 0, weights")
    assert np.isnan(got.accepted_mean[0][w[..., 0] == 0]).all()
    ones = erd.erd_volume(dwi, b0, (1, 2, 3), B, rule=0)
    _check_against_restatement(ones, V.restate(dwi, b0, (1, 2, 3), B, rule=0), "rule 0, no weights")
    assert (ones.accept == 1).all() and V.same_bits(ones.accepted_mean, ones.direction_mean)
    edited = erd.erd_volume(dwi, b0, (1, 2, 3), B, rule=1).accept                 # a rule-1 result fed back, as an edited case.accept
    again = erd.erd_volume(dwi, b0, (1, 2, 3), B, rule=0, accept=edited)
    assert V.same_bits(again.accepted_mean, erd.erd_volume(dwi, b0, (1, 2, 3), B, rule=1).accepted_mean)


@pytest.mark.gpu
def test_a_volume_equals_its_slices():
    from mri_super_resolution_amd import erd
    dwi, b0 = V.volume_case((5, 7, 3, 12), (4, 4, 4), seed=33)
    emap = np.random.default_rng(2).random((5, 7, 3)) - 0.4
    for rule, em in ((1, None), (2, emap)):
        whole = erd.erd_volume(dwi, b0, (4, 4, 4), B, rule=rule, erd_map=em, per_acquisition_adc=True)
        for s in range(3):
            one = erd.erd_volume(dwi[:, :, s], b0[:, :, s], (4, 4, 4), B, rule=rule, erd_map=None if em is None else em[:, :, s],
                                 per_acquisition_adc=True)
            assert np.array_equal(one.accept, whole.accept[:, :, s]) and V.same_bits(one.adc, whole.adc[:, :, s])
            for name in ("direction_mean", "accepted_mean", "direction_adc", "accepted_adc"):
                assert V.same_bits(getattr(one, name), getattr(whole, name)[:, :, :, s]), (rule, s, name)


# ---- the driver and the entry script on a synthetic patient ---------------------------------------------------------------------------
HOST_ROUNDINGS = 4      # the mean of a 2 x 2 square: three additions and a division, each rounded on slightly different values


def _contrast_bounds(case, image, focus, ulps):
    """First-order bounds on |delta C| and |delta CNR| of contrast.calculate_contrast when every pixel of ``image`` may move by
    ``ulps`` ULPs: a pixel, hence a square's mean and (the standard deviation being 1-Lipschitz in the largest deviation) its
    standard deviation, moves by at most e = (ulps + HOST_ROUNDINGS) 2^-52 max|v|.  C = m1 / (m2 + 1e-7) then moves by at most
    |C| (e / |m1| + e / |m2 + 1e-7|) and CNR = gap / pooled by at most CNR (2 e / gap + 2 e / pooled).  ulps = 0: (0, 0)."""
    from mri_super_resolution_amd.contrast import _square
    if ulps == 0:
        return 0.0, 0.0
    lesion, mirror = (_square(image, p, focus, 1) for p in (case.cancer_loc, case.contralateral_loc))
    e = (ulps + HOST_ROUNDINGS) * 2.0 ** -52 * max(np.abs(lesion).max(), np.abs(mirror).max())
    m1, m2 = lesion.mean(), mirror.mean()
    gap, pooled = abs(m1 - m2), np.sqrt(np.std(lesion) ** 2 + np.std(mirror) ** 2)
    return abs(m1 / (m2 + 1e-7)) * (e / abs(m1) + e / abs(m2 + 1e-7)), gap / pooled * (2 * e / gap + 2 * e / pooled)


@pytest.fixture(scope="module")
def patient(tmp_path_factory, golden):
    """pat07_volume.npz as test_erd.py::test_master_script_with_auto_erd builds its patient -- six acquisitions in groups
    (2, 2, 2), a signal dropout planted in acquisition 2 -- on four slices (9 .. 12 of the volume; the cancer slice 11 is slice 2),
    with one change.  Six acquisitions that differ by noise alone split 5 + 1 or 4 + 2 at most pixels and rule 1 then rejects the
    minority, so 'nothing is rejected in the untouched slices' cannot hold for such data.  Here acquisitions 3 .. 5 lie a quarter
    above acquisitions 0 .. 2 (plus 0.05, so that background pixels split the same way) and the noise is 0.1 %: every untouched
    pixel splits 3 + 3 and keeps everything, and the dropout (x 0.2) leaves acquisition 2 alone against five."""
    from mri_super_resolution_amd import matio
    tmp = tmp_path_factory.mktemp("david")
    vol = golden("pat07_volume.npz")["vol"].astype(np.float64)[:, :, 9:13]
    rng = np.random.default_rng(6)
    high = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    dwi = np.stack([0.4 * vol * (1 + 0.25 * high[k]) * (1 + 0.001 * rng.standard_normal(vol.shape)) + 0.05 * high[k] for k in range(6)],
                   axis=-1)
    dwi[50:70, 50:70, 2, 2] *= 0.2
    data_dir = tmp / "anon_data"
    data_dir.mkdir()
    matio.savemat(str(data_dir / "pat07_alldata.mat"), {"data": dwi.astype(np.float32)})
    matio.savemat(str(data_dir / "pat07_mean_b0.mat"), {"data_mean_b0": vol.astype(np.float32)})
    spec = [{"pt_id": "18-1681-07", "b": 900, "cancer_loc": [60, 70], "contralateral_loc": [60, 55], "noise": [45, 45],
             "cancer_slice": 2, "acquisitions": [2, 2, 2]}]
    with open(str(tmp / "cases.json"), "w") as fh:
        json.dump(spec, fh)
    return tmp


def _load(patient):
    from mri_super_resolution_amd.scripts import david as david_script
    from mri_super_resolution_amd.scripts.master import load_cases
    args = david_script.build_parser().parse_args(["--data_dir", str(patient / "anon_data"), "--cases", str(patient / "cases.json")])
    return load_cases(args)


@pytest.mark.gpu
def test_david_script_on_all_slices(patient):
    from mri_super_resolution_amd import matio, reports
    from mri_super_resolution_amd.contrast import calculate_contrast
    from mri_super_resolution_amd.scripts import david as david_script
    cases = _load(patient)
    case = cases[0]
    args = david_script.build_parser().parse_args(["--out_folder", str(patient / "exp"), "--experiment_name", "d1", "--slices", "all",
                                                   "--save_maps"])
    out = david_script.run(args, cases)
    want_acc = np.ones(case.dwi.shape, dtype=int)
    want_acc[50:70, 50:70, 2, 2] = 0
    assert np.array_equal(case.accept, want_acc)                  # the dropout where it was planted, nothing anywhere else
    rows = reports.read_csv(out["csv"])
    assert len(rows) == 3 * (2 * 2 * 2 + 2 * 4) == 48 and list(rows[0]) == ["patient", "image", "direction", "acquisition", "metric",
                                                                             "performance"]
    # the restatement on a window of the cancer slice that holds the three landmarks (focus = 40)
    f0, f1 = 40, 80
    dwi = np.asarray(case.dwi, np.float64)[f0:f1, f0:f1, 2, :]
    b0 = np.asarray(case.b0, np.float64)[f0:f1, f0:f1, 2]
    want = V.restate(dwi, b0, (2, 2, 2), case.b, rule=1)
    assert np.array_equal(want.accept, want_acc[f0:f1, f0:f1, 2, :])
    worst = 0.0
    for r in rows:
        g = "xyz".index(r["direction"])
        if r["acquisition"] == "mean":
            image, ulps = {"DWI": (want.direction_mean[g], 0), "ADC": (want.direction_adc[g], V.ADC_ULP),
                           "DWI_ERD": (want.accepted_mean[g], 0), "ADC_ERD": (want.accepted_adc[g], V.ADC_ULP)}[r["image"]]
        else:
            a = int(r["acquisition"])
            assert a // 2 == g
            image, ulps = {"DWI": (case.dwi[f0:f1, f0:f1, 2, a], 0), "ADC": (want.adc[..., a], V.ADC_ULP)}[r["image"]]     # (float32, as read)
        k = ("C", "CNR").index(r["metric"])
        value, got = calculate_contrast(case, 1, image, f0)[k], float(r["performance"])
        bound = _contrast_bounds(case, image, f0, ulps)[k]
        assert np.isfinite(value) and abs(got - value) <= bound, (r, value, bound)
        worst = max(worst, abs(got - value) / bound) if bound else worst
    print(f"david.csv: largest |difference| / bound over the ADC rows {worst:.3f}")
    perf = lambda image, d: [float(r["performance"]) for r in rows if r["image"] == image and r["direction"] == d           # noqa: E731
                             and r["acquisition"] == "mean"]
    assert perf("DWI_ERD", "y") != perf("DWI", "y") and perf("ADC_ERD", "y") != perf("ADC", "y")    # y holds acquisition 2
    assert perf("DWI_ERD", "x") == perf("DWI", "x") and perf("DWI_ERD", "z") == perf("DWI", "z")
    maps = matio.loadmat(out["maps"][0])
    assert out["maps"][0].endswith("david_07.mat") and maps["direction_mean"].shape == (3, 128, 128, 4)
    assert maps["adc"].shape == (128, 128, 4, 6) and np.array_equal(maps["accept"], want_acc)
    assert np.array_equal(np.asarray(maps["slices"]).reshape(-1), [0, 1, 2, 3])
    assert V.same_bits(maps["accepted_mean"][:, f0:f1, f0:f1, 2], want.accepted_mean)
    # the default --slices cancer writes the same table
    cases2 = _load(patient)
    out2 = david_script.run(david_script.build_parser().parse_args(["--out_folder", str(patient / "exp"), "--experiment_name", "d2"]),
                            cases2)
    assert open(out2["csv"]).read() == open(out["csv"]).read() and out2["maps"] == []
    assert np.array_equal(cases2[0].accept, want_acc)


@pytest.mark.gpu
def test_apply_auto_erd_volume_on_the_cancer_slice(patient):
    from mri_super_resolution_amd import erd
    case = _load(patient)[0]
    erd.apply_auto_erd_volume(case, 1, "cancer")
    assert np.array_equal(case.accept[:, :, 2, :], E.auto_erd(case.dwi[:, :, 2, :], 1))
    assert case.accept[:, :, [0, 1, 3], :].all() and (case.accept[:, :, 2, :] == 0).any()
    with pytest.raises(ValueError, match="--erd 2 needs the patient's ERD map"):
        erd.apply_auto_erd_volume(case, 2, "all")
    case.erd = np.full(case.dwi.shape[:3], -np.inf, np.float32)                  # the published maps hold -inf
    case.erd[:, :64, 1] = 1.0
    before = case.accept.copy()
    erd.apply_auto_erd_volume(case, 2, [1, 3])
    assert np.array_equal(case.accept[:, :, [0, 2], :], before[:, :, [0, 2], :]) and case.accept[:, 64:, 1].all()
    assert case.accept[:, :, 3].all() and (case.accept[:, :64, 1] == 0).any()
