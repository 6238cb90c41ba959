"""CPU: whole-volume AutoERD (erd.erd_volume, csrc/erd_volume.hip) -- the float64 restatement on a hand-computed case, the
extent identity the kernel rests on (a chain walk on (min, max) extents gives the oracle's partition), the entry point's host-side
argument checks, and the david script's parser, CSV header and row order."""
import ctypes
import math
import types

import numpy as np

from oracle import erd_oracle as E
from tests import erd_volume_common as V
from mri_super_resolution_amd import _build, _lib


def test_restatement_on_a_hand_computed_case():
    # two pixels, four acquisitions in groups (3, 1), rule 1 (a cluster of >= 8/3 acquisitions rejects the other)
    dwi = np.array([[40.0, 44.0, 42.0, 5.0],        # {40, 44, 42} | {5}: 3 >= 2.67 rejects acquisition 3 = the whole of group 1
                    [20.0, 22.0, 60.0, 62.0]])      # {20, 22} | {60, 62}: 2 < 2.67, nothing is rejected
    b0 = np.array([100.0, 50.0])
    r = V.restate(dwi, b0, (3, 1), 1000, rule=1)
    assert r.accept.tolist() == [[1, 1, 1, 0], [1, 1, 1, 1]]
    assert r.direction_mean.tolist() == [[42.0, 34.0], [5.0, 62.0]]
    assert r.accepted_mean[0].tolist() == [42.0, 34.0] and r.accepted_mean[1, 1] == 62.0
    assert np.isnan(r.accepted_mean[1, 0]) and np.isnan(r.accepted_adc[1, 0])           # 0 / 0, and its ADC
    want = lambda v, b: -math.log(v / (b + 1e-7) + 1e-7) / 1000 * 1000                   # noqa: E731  (ONE factor 1000)
    assert math.isclose(r.direction_adc[0, 0], want(42.0, 100.0), rel_tol=1e-15)
    assert math.isclose(r.direction_adc[1, 0], want(5.0, 100.0), rel_tol=1e-15)
    assert math.isclose(r.accepted_adc[0, 1], want(34.0, 50.0), rel_tol=1e-15)
    assert math.isclose(r.adc[1, 2], want(60.0, 50.0), rel_tol=1e-15) and r.adc.shape == (2, 4)
    assert abs(r.direction_adc[0, 0] - 0.8675005677) < 1e-6                              # -ln(0.42) by hand, eps apart
    # rule 0: supplied weights are used as they are; no weights = everything accepted
    w = np.array([[1.0, 0.0, 0.5, 1.0], [0.0, 0.0, 0.0, 1.0]])
    r0 = V.restate(dwi, b0, (3, 1), 1000, rule=0, accept=w)
    assert r0.accepted_mean[0, 0] == (40.0 + 21.0) / 1.5 and np.isnan(r0.accepted_mean[0, 1]) and r0.accepted_mean[1, 1] == 62.0
    r1 = V.restate(dwi, b0, (3, 1), 1000, rule=0)
    assert V.same_bits(r1.accepted_mean, r1.direction_mean) and (r1.accept == 1).all()
    # a non-finite pixel keeps everything; b0 == 0 with dwi == 0 gives the finite -log(eps) value; a negative value gives NaN
    x = np.array([[1.0, np.nan, 3.0, 50.0], [0.0, 0.0, 0.0, -1.0]])
    r2 = V.restate(x, np.array([10.0, 0.0]), (3, 1), 900, rule=1)
    assert r2.accept[0].tolist() == [1, 1, 1, 1]
    assert math.isclose(r2.direction_adc[0, 1], -math.log(1e-7) / 900 * 1000, rel_tol=1e-15) and np.isnan(r2.adc[1, 3])
    assert V.max_ulp([1.0, np.nan, -0.0], [np.nextafter(1.0, 2.0), np.nan, 0.0]) == 1 and V.max_ulp([np.nan], [1.0]) == 2 ** 62
    assert V.ADC_ULP == 4


def _same_partition(m, want):
    return m is not None and (np.array_equal(m, want) or np.array_equal(~m, want))


def test_extent_walk_gives_the_oracle_partition_on_the_sklearn_fixture(golden):
    g = golden("erd.npz")
    count = 0
    for v, n, lab in zip(g["values"], g["lengths"], g["labels"]):
        x, lab = v[:n], lab[:n]
        m = V.extent_two_clusters(x)
        assert _same_partition(m, lab == lab[0]), (x, lab, m)                    # sklearn's own labels
        assert _same_partition(m, E.complete_linkage_two_clusters(x)), x
        count += 1
    assert count == 2460


def test_extent_walk_gives_the_oracle_partition_on_tie_rich_long_samples():
    rng = np.random.default_rng(1732)
    count = 0
    for n in range(17, 33):
        for kind in range(12):
            if kind % 4 == 0:
                x = np.round(rng.normal(300.0, 6.0, n))                           # integer-valued: many equal distances
            elif kind % 4 == 1:
                x = rng.choice([100.0, 101.0, 103.0, 400.0], n)                   # few-valued
            elif kind % 4 == 2:
                x = rng.normal(0.0, 1.0, n).astype(np.float32).astype(np.float64)  # float32-valued
            else:
                x = np.round(rng.uniform(0.0, 3.0, n), 1)                         # decimal steps: inexact differences that tie
            assert _same_partition(V.extent_two_clusters(x), E.complete_linkage_two_clusters(x)), x
            count += 1
    assert count == 16 * 12
    assert V.extent_two_clusters([1e308, -1e308]) is None                        # every extent overflows: no neighbour, no index


def test_erd_volume_arguments_are_checked_on_the_host():
    assert "erd_volume.hip" in _build.SOURCES and "-ffp-contract=off" in _build.SOURCE_FLAGS["erd_volume.hip"]
    lib = _lib.lib()
    fake = lambda k: ctypes.c_void_p(0x7000_0000_0000 + 4096 * k)      # noqa: E731  never dereferenced: every call fails in validation
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                      # noqa: E731
    INV = _lib.INR_E_INVALID

    def call(values=fake(6), b0=fake(7), n_pixels=100, n=12, groups=ints(4, 4, 4), G=3, b=900.0, rule=1, accept_in=None, adc=fake(5)):
        return lib.inr_auto_erd_volume(fake(0), fake(1), fake(2), fake(3), fake(4), adc, values, b0, fake(8), accept_in, n_pixels, n, groups,
                                  G, b, rule, None)

    assert call(values=None) == INV and b"null pointer" in lib.inr_last_error()
    assert call(b0=None) == INV and b"b0" in lib.inr_last_error()
    assert call(groups=None) == INV and b"null pointer" in lib.inr_last_error()
    assert call(n_pixels=-1) == INV and b"pixel count" in lib.inr_last_error()
    for n, groups in ((1, ints(1)), (33, ints(33)), (0, ints(1))):
        assert call(n=n, groups=groups, G=1) == INV and b"acquisitions" in lib.inr_last_error(), n
    for rule in (-1, 3):
        assert call(rule=rule) == INV and b"rule must be" in lib.inr_last_error()
    for G in (0, 9):
        assert call(groups=ints(*([1] * 9)), G=G) == INV and b"groups" in lib.inr_last_error()
    assert call(groups=ints(4, 4, 3)) == INV and b"sum to 11" in lib.inr_last_error()
    assert call(groups=ints(4, 4, 5)) == INV and b"sum to 13" in lib.inr_last_error()
    assert call(groups=ints(12, 0), G=2) == INV and b"size 0" in lib.inr_last_error()
    assert call(groups=ints(13, -1), G=2) == INV and b"size -1" in lib.inr_last_error()
    assert call(b=0.0) == INV and b"b must not be 0" in lib.inr_last_error()
    assert call(accept_in=fake(9)) == INV and b"rule 0" in lib.inr_last_error()
    # 0 pixels is a no-op that touches no pointer (and, here, no device)
    assert call(n_pixels=0) == 0 and call(n_pixels=0, rule=0, accept_in=fake(9)) == 0


def test_david_script_parser_and_csv_rows(tmp_path):
    from mri_super_resolution_amd import drivers, reports
    from mri_super_resolution_amd.scripts import david as david_script
    args = david_script.build_parser().parse_args([])
    assert (args.out_folder, args.experiment_name, args.erd, args.slices, args.save_maps, args.cases) == \
        ('../experiments/', 'david', 1, 'cancer', False, None)
    args = david_script.build_parser().parse_args(["--out_folder", "o", "--experiment_name", "e", "--data_dir", "d", "--cases", "c.json",
                                                   "--erd", "2", "--slices", "all", "--save_maps"])
    assert (args.out_folder, args.experiment_name, args.data_dir, args.cases, args.erd, args.slices, args.save_maps) == \
        ("o", "e", "d", "c.json", 2, "all", True)
    # rows from the restatement's maps of a small synthetic patient: two slices, six acquisitions in groups (2, 2, 2)
    rng = np.random.default_rng(5)
    dwi = np.round(rng.uniform(200.0, 400.0, (16, 16, 2, 6)))
    b0 = np.round(rng.uniform(800.0, 900.0, (16, 16, 2)))
    case = types.SimpleNamespace(pt_id="18-1681-07", b=900, cancer_loc=(8, 10), contralateral_loc=(8, 4), noise=(3, 3), cancer_slice=1,
                                 acquisitions=np.asarray([2, 2, 2]), dwi=dwi, b0=b0)
    res = V.restate(dwi, b0, case.acquisitions, case.b, rule=1)
    rows = drivers.david_rows(case, res, 1)
    assert len(rows) == 3 * (2 * 2 * 2 + 2 * 4) == 48
    want = []
    for d, name in enumerate("xyz"):
        for acq in (2 * d, 2 * d + 1):
            want += [(im, name, acq, m) for m in ("C", "CNR") for im in ("DWI", "ADC")]
        want += [(im, name, "mean", m) for m in ("C", "CNR") for im in ("DWI", "ADC", "DWI_ERD", "ADC_ERD")]
    assert [r[:4] for r in rows] == want
    from mri_super_resolution_amd.contrast import calculate_contrast
    assert rows[0][4] == calculate_contrast(case, 1, dwi[:, :, 1, 0], 0)[0]
    assert rows[3][4] == calculate_contrast(case, 1, res.adc[:, :, 1, 0], 0)[1]
    assert rows[8 + 7][4] == calculate_contrast(case, 1, res.accepted_adc[0, :, :, 1], 0)[1]
    csv = reports.DavidCsv(str(tmp_path / "exp" / "david.csv"))
    csv.rows("07", rows)
    lines = open(csv.path).read().splitlines()
    assert lines[0] == "patient,image,direction,acquisition,metric,performance" and len(lines) == 49
    assert lines[1] == f"07,DWI,x,0,C,{rows[0][4]}" and lines[9].startswith("07,DWI,x,mean,C,") and lines[48].startswith("07,ADC_ERD,z,mean,CNR,")
    back = reports.read_csv(csv.path)
    assert np.array_equal([float(r["performance"]) for r in back], [float(r[4]) for r in rows], equal_nan=True)     # repr round trip
