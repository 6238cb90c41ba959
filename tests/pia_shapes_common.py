"""The case table of the PIA kernels' shape classes, and the host rules of csrc/pia.hip restated in plain Python so that the
table can prove which kernel form, split count and reduction each of its cases runs.

Every rule below names the lines it restates.  `classes_of(case)` walks the launches of one case the way
`pia_forward_layers` / `pia_backward_layers` / `inr_pia_forward` issue them and returns the set of classes the case reaches;
tests/test_pia_shapes_cpu.py asserts that the union over `CASES` is `ALL_CLASSES`, so an edit of the table that loses a class
fails on the CPU.  tools/gen_golden_pia_net.py --shapes writes tests/golden/pia_net_shapes.npz for the same table.
"""
from dataclasses import dataclass

import numpy as np
import torch

import pia_net_common as C

# ---- the host rules ------------------------------------------------------------------------------------------------------------
PIA_BK = 16                 # pia.hip:30
FIN_GROUP = 32              # common.h:196
FIN_TALL = 4 * FIN_GROUP    # common.h:197
HEAD_WAVE_CAP = 1024        # pia.hip:502
FWD_ROWS_PER_WAVE = 16      # pia.hip:507-509
FWD_CHUNK = 32768           # pia_net.py: pia_forward(chunk_rows=32768)


def cdiv(a, b):
    return (a + b - 1) // b


def pia_big(M, N, z):
    """pia.hip:198-200: 128 x 128 tiles once they fill the chip."""
    return M >= 128 and N >= 128 and cdiv(M, 128) * cdiv(N, 128) * z >= 256


def dw_big(n, out_f, in_f):
    """pia.hip:205 (and the launches at pia.hip:644, 673): the tile of a parameter-gradient GEMM."""
    return out_f >= 128 and in_f >= 128 and n >= 4096


def pia_dw_splits(n, out_f, in_f, nbatch):
    """pia.hip:204-214 -> (splits, what limited them: 'rows', 'tiles' or 'cap')."""
    t = 128 if dw_big(n, out_f, in_f) else 64
    tiles = cdiv(out_f, t) * cdiv(in_f, t) * nbatch
    by_tiles = cdiv(512, tiles)
    by_rows = cdiv(n, 64)
    s = max(1, min(by_tiles, by_rows, 128))
    why = "cap" if min(by_tiles, by_rows) > 128 else "rows" if by_rows < by_tiles else "tiles" if by_tiles < by_rows else "rows+tiles"
    return s, why


def dw_split_ranges(K, splits):
    """pia.hip:60-66: the [kbeg, kend) of every split; the chunk is rounded up to PIA_BK rows, so trailing splits can be empty."""
    chunk = cdiv(cdiv(K, splits), PIA_BK) * PIA_BK
    out = []
    for s in range(splits):
        kbeg = s * chunk
        kend = min(kbeg + chunk, K)
        out.append((min(kbeg, kend), kend))
    return out


def pia_head_waves(n):
    """pia.hip:500-504: waves of the training row kernel (each leaves a slab row), capped."""
    return cdiv(min(cdiv(n, 4), HEAD_WAVE_CAP), 4) * 4


def pia_head_waves_fwd(n):
    """pia.hip:510-514: the forward-only row kernel writes no slabs, nothing caps its grid."""
    return cdiv(cdiv(n, FWD_ROWS_PER_WAVE), 4) * 4


def head_idle_waves(n, waves):
    """pia.hip:256-257: wave w owns rows [w per, min((w + 1) per, n)); how many own none."""
    per = cdiv(n, waves)
    return sum(1 for w in range(waves) if w * per >= n)


def fin_stages(nslabs):
    """common.h:196-197, kernels.hip:381-383 and 420-422 -> (stages, groups, rows of the last group)."""
    if nslabs > FIN_TALL:
        groups = cdiv(nslabs, FIN_GROUP)
        return 2, groups, nslabs - (groups - 1) * FIN_GROUP
    return 1, 1, nslabs


# ---- the table -----------------------------------------------------------------------------------------------------------------
SHAPES = {
    "A": (32, 64, 128, 256, 512),
    "B": (48, 80, 144, 256),
    "C": (16, 48, 272, 512),
    "D": (80, 16, 112, 48, 176, 64, 208, 256),
    "W512": (512,),
    "W256": (256,),
}
TABLES = {
    "4x4": (C.B_VALUES, C.TE_VALUES),
    "2x8": ((0, 1000), (0, 13, 33, 53, 73, 93, 118, 143)),
    "8x2": ((0, 150, 300, 500, 750, 1000, 1250, 1500), (0, 93)),
}
FUNCTIONALS = ("signal", "D", "T2", "v", "all")


@dataclass(frozen=True)
class Case:
    shape: str
    rows: int
    kind: str = "train"          # train | forward | functional
    table: str = "4x4"
    functional: str = ""
    seed: int = 0                # NumPy seed of the get_batch pool

    @property
    def name(self):
        tail = "" if self.table == "4x4" else f"_{self.table}"
        tail += f"_{self.functional}" if self.functional else ""
        return f"{self.kind}_{self.shape}_{self.rows}{tail}"

    @property
    def hidden(self):
        return SHAPES[self.shape]

    @property
    def tables(self):
        return TABLES[self.table]


def _table():
    cases = []
    for shape in ("B", "C"):
        for rows in (1, 17, 63, 65, 129):
            cases.append(Case(shape, rows))
    for rows in (1, 65, 513):
        cases.append(Case("D", rows))
    for rows in (513, 4096, 8269, 16461):
        cases.append(Case("A", rows))
    cases.append(Case("B", 8269))
    cases.append(Case("A", 130, table="2x8"))
    cases.append(Case("A", 130, table="8x2"))
    cases.append(Case("A", 32773, kind="forward"))
    for shape in ("W512", "W256"):
        for rows in (1, 65):
            cases.append(Case(shape, rows, kind="forward"))
    for shape in ("A", "B"):
        for f in FUNCTIONALS:
            cases.append(Case(shape, 129, kind="functional", functional=f))
    # one seed per case; the five functionals of a shape share theirs (batch and weights), so that their gradients add up
    return tuple(Case(c.shape, c.rows, c.kind, c.table, c.functional, seed=2000 + ord(c.shape[0]) if c.functional else 1000 + i)
                 for i, c in enumerate(cases))


CASES = _table()
TRAIN_CASES = tuple(c for c in CASES if c.kind == "train")
FORWARD_CASES = tuple(c for c in CASES if c.kind == "forward")
FUNCTIONAL_CASES = tuple(c for c in CASES if c.kind == "functional")
UNFILTERED = next(c for c in CASES if c.shape == "C" and c.rows == 65 and c.kind == "train")   # its batch also runs without the kink filter
BY_NAME = {c.name: c for c in CASES}

# what the kernels and the host rules distinguish ...
CORE_CLASSES = (
    "gemm_fwd_64", "gemm_fwd_128", "gemm_dx_64", "gemm_dx_128", "gemm_dw_64", "gemm_dw_128",
    "head_q1", "head_q2", "head_idle_wave", "head_wave_cap",
    "slab_one_stage", "slab_two_stage", "slab_ragged_last_group",
    "dw_splits_by_rows", "dw_splits_by_tiles", "dw_splits_capped_128", "dw_empty_split", "dw_single_partial_kstep",
    "tile_columns_cut",
)
# ... and, beside them, which layer width meets the big tiles, depth, width order, tables, chunking
EXTRA_CLASSES = (
    "gemm_fwd_128_n128", "gemm_fwd_128_n256", "gemm_fwd_128_n512", "gemm_fwd_128_heads", "gemm_dx_128_n256", "gemm_dx_128_heads",
    "gemm_dw_128_cut", "width_odd_multiple_of_16", "encoder_8_layers", "encoder_1_layer", "widths_descending",
    "table_2x8", "table_8x2", "forward_tail_chunk", "external_gradient_null", "external_gradient_g_D",
    "row_tile_one_short", "row_tile_one_over",
)
ALL_CLASSES = CORE_CLASSES + EXTRA_CLASSES


def _gemm(out, epi, M, N, big, tag=""):
    """One GEMM launch: the instantiation, and whether N leaves the last tile column cut (`n < p.N`, pia.hip:102, 162).

    Tile columns themselves start at multiples of the tile width; what varies is where the matrix ends inside the last one.  A
    width that is an odd multiple of 16 ends it at a non-multiple of 64, which is where the four-wide loads lean on the guard
    of their first element alone (pia.hip:77-80)."""
    t = 128 if big else 64
    out.add(f"gemm_{epi}_{t}")
    if N % t and N > t:                                         # a cut tile column behind a whole one
        out.add("tile_columns_cut")
        if big and epi == "dw":
            out.add("gemm_dw_128_cut")
    if big and tag:
        out.add(f"gemm_{epi}_128_{tag}")


def _forward_launches(out, hidden, n):
    for width in hidden:                                        # pia.hip:600-611
        _gemm(out, "fwd", n, width, pia_big(n, width, 1), f"n{width}" if width in (128, 256, 512) else "")
    H = hidden[-1]
    _gemm(out, "fwd", n, H, pia_big(n, H, 3), "heads")          # pia.hip:612-622
    out.add("head_q2" if H == 512 else "head_q1")               # pia.hip:586-589


def classes_of(case):
    hidden, n = case.hidden, case.rows
    out = set()
    ins = (16,) + tuple(hidden[:-1])
    H = hidden[-1]
    if any((w // 16) % 2 == 1 and w % 16 == 0 for w in hidden):
        out.add("width_odd_multiple_of_16")
    if len(hidden) == 8:
        out.add("encoder_8_layers")
    if len(hidden) == 1:
        out.add("encoder_1_layer")
    if any(b < a for a, b in zip(hidden, hidden[1:])):
        out.add("widths_descending")
    if case.table != "4x4":
        out.add(f"table_{case.table}")
    if n % 64 == 63:
        out.add("row_tile_one_short")                           # the last row of a 64-row tile masked by `m < p.M` (pia.hip:93, 167)
    if n % 64 == 1 and n > 64:
        out.add("row_tile_one_over")                            # a row tile that holds one row
    if case.kind == "forward":                                  # pia.hip:810-820 under pia_forward's default chunk
        for r in range(0, n, FWD_CHUNK):
            rows = min(FWD_CHUNK, n - r)
            _forward_launches(out, hidden, rows)
            if rows < FWD_CHUNK and r > 0:
                out.add("forward_tail_chunk")
        return out
    _forward_launches(out, hidden, n)
    # the row kernel in its training form (pia.hip:549, 861, 885) and the reduction of its slabs (pia.hip:707-712)
    waves = pia_head_waves(n)
    if head_idle_waves(n, waves):
        out.add("head_idle_wave")
    if cdiv(n, 4) > HEAD_WAVE_CAP:
        out.add("head_wave_cap")
    stages, _, last = fin_stages(waves)
    out.add("slab_two_stage" if stages == 2 else "slab_one_stage")
    if stages == 2 and last != FIN_GROUP:
        out.add("slab_ragged_last_group")
    # parameter gradients: the heads' (pia.hip:631-645), then every encoder layer's (pia.hip:662-674)
    dws = [(H, H, 3)] + [(o, i, 1) for o, i in zip(hidden, ins)]
    for o, i, nb in dws:
        _gemm(out, "dw", o, i, dw_big(n, o, i))
        s, why = pia_dw_splits(n, o, i, nb)
        if "rows" in why:
            out.add("dw_splits_by_rows")
        if why == "tiles":
            out.add("dw_splits_by_tiles")
        if why == "cap":
            out.add("dw_splits_capped_128")
        ranges = dw_split_ranges(n, s)
        assert ranges[-1][1] == n and all(a[1] == b[0] or b[0] == b[1] for a, b in zip(ranges, ranges[1:]))
        if any(b == e for b, e in ranges):
            out.add("dw_empty_split")
        assert stages and fin_stages(s)[0] == 1                 # at most 128 slabs: one stage (pia.hip:202-203)
    if n < PIA_BK:
        out.add("dw_single_partial_kstep")
    # input gradients: the heads' three-segment product (pia.hip:646-659), then layers top .. 1 (pia.hip:675-687)
    _gemm(out, "dx", n, H, pia_big(n, H, 1), "heads")
    for l in range(len(hidden) - 1, 0, -1):
        _gemm(out, "dx", n, ins[l], pia_big(n, ins[l], 1), f"n{ins[l]}" if ins[l] == 256 else "")
    if case.kind == "functional":
        if case.functional != "all":
            out.add("external_gradient_null")
        if case.functional in ("D", "all"):
            out.add("external_gradient_g_D")
    return out


def launch_counts(case, fused):
    """The counters of ops.pia_launch_counts() after one training pass (autograd pair: forward + backward, or one fused step)."""
    L = len(case.hidden)
    return {"pia_fwd": L + 1, "pia_dx": L, "pia_dw": L + 1, "pia_head": 1 if fused else 2}


# ---- inputs --------------------------------------------------------------------------------------------------------------------
POOL_EXTRA = 1024


def pool_rows(rows):
    """rows + 1024, as long as a pool with the admitted 10 % of flagged rows still holds `rows` clean ones (up to 9,216 rows);
    beyond, rows + rows / 8.  (The default shape flags about 7 % of a batch: a fixed 1,024 spare rows run out at 16,461.)"""
    return rows + (POOL_EXTRA if MAX_FLAGGED * (rows + POOL_EXTRA) <= POOL_EXTRA else rows // 8)
MAX_FLAGGED = 0.10
PIDS_SEED = 11


def case_inputs(case, host_params, get_batch, filtered=True):
    """-> x [rows, 16] float32, pids [rows, 16] float32, rows of the pool that `kink_rows` flagged (None when unfiltered).

    Gradient cases take the first `rows` rows of a seeded pool of `pool_rows(rows)` that `kink_rows` does not flag; forward-only
    cases (and `filtered=False`) take the seeded batch as it comes."""
    np.random.seed(case.seed)
    if case.kind == "forward" or not filtered:
        x = get_batch(case.rows, 0.02)[0]
        return x.contiguous(), torch.from_numpy(C.pids_map(case.rows, seed=PIDS_SEED)), None
    pool = get_batch(pool_rows(case.rows), 0.02)[0]
    flagged = C.kink_rows(host_params, pool)
    x = pool[~flagged][:case.rows].contiguous()
    assert x.shape[0] == case.rows, "the pool ran out of rows off the LeakyReLU kinks"
    return x, torch.from_numpy(C.pids_map(case.rows, seed=PIDS_SEED)), int(flagged.sum())


def functional_weights(rows, seed):
    """Seeded weights of the linear functionals sum(w * out): float32 for signal, T2 and v, float64 for D -- the dtypes of the
    outputs, so that autograd hands the backward kernel g_signal / g_T2 / g_v in float32 and g_D in float64."""
    rng = np.random.default_rng(seed)
    return {"signal": torch.from_numpy((rng.standard_normal((rows, 16)) * 1e-3).astype(np.float32)),
            "D": torch.from_numpy(rng.standard_normal((rows, 3))),
            "T2": torch.from_numpy((rng.standard_normal((rows, 3)) * 1e-2).astype(np.float32)),
            "v": torch.from_numpy(rng.standard_normal((rows, 3)).astype(np.float32))}


def functional_terms(which):
    return ("signal", "D", "T2", "v") if which == "all" else (which,)


def functional64(which, w):
    """The functional as `loss_and_grads64(functional=...)` takes it."""
    def f(signal, D, T2, v):
        outs = {"signal": signal, "D": D, "T2": T2, "v": v}
        return sum((w[k].double() * outs[k]).sum() for k in functional_terms(which))
    return f


def flat_grad_sample(grads, k=997):
    """The fixture's gradient record: every 997th element of the gradients laid end to end (a prime stride walks every tensor
    and column), and each tensor's L1 norm, which moves with any of its elements."""
    flat = np.concatenate([np.asarray(g, dtype=np.float64).reshape(-1) for g in grads])
    return flat[::k], np.array([np.abs(np.asarray(g, dtype=np.float64)).sum() for g in grads])


def params_sha(params):
    return C.sha(np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in params]))


def bounds(ref_err, factor=4.0):
    """Per tensor: factor x max(its own ref_err, the median ref_err of the case's tensors of the same kind).  One tensor's
    ref_err is a single draw of rounding luck; the median keeps a lucky-small draw from becoming an accidental bound."""
    e = np.asarray(ref_err, dtype=np.float64)      # NaN: a gradient the functional does not reach (zero on both sides, no bound)
    return factor * np.maximum(e, np.nanmedian(e))


# ---- detect_PIDS_slice inputs ----------------------------------------------------------------------------------------------------
PIDS_PIXELS = (1, 255, 256, 257)


def pids_slice_input(n, seed=21):
    """S [1, n, 4 (b), 4 (TE)] float64: decaying signals of order 1000 with, walking round the pixels, zeros, negatives (the
    logarithm of the ADC fit is NaN there: both ADC flags come out 0), exact ties, and neighbours just below / above an
    integer.  Pixel i takes edit i % 8; edit 0 leaves the pixel alone."""
    rng = np.random.default_rng(seed + n)
    b = np.array(C.B_VALUES, dtype=np.float64)[None, :, None]
    te = np.array(C.TE_VALUES, dtype=np.float64)[None, None, :]
    S = 1000 * rng.uniform(0.3, 1.0, (n, 1, 1)) * np.exp(-b / 1000 * rng.uniform(0.3, 3.0, (n, 1, 1))) * np.exp(-te / rng.uniform(30, 500, (n, 1, 1)))
    S = S + rng.normal(0, 10.0, S.shape)
    for i in range(n):
        e = (i + (n == 1)) % 8                      # the single pixel of n == 1 takes edit 1
        if e == 1:
            S[i, 1, 0] = 0.0                        # a zero on the ADC line and in both decay maps
            S[i, 2, 2] = 0.0
        elif e == 2:
            S[i, 2, 0] = -3.5                       # a negative on the ADC line: log -> NaN
            S[i, 0, 3] = -0.25                      # truncates to -0
        elif e == 3:
            S[i, 1, 2] = S[i, 1, 1]                 # tie along TE
            S[i, 3, 1] = S[i, 2, 1]                 # tie along b
        elif e == 4:
            S[i, 0, 1] = np.floor(S[i, 0, 1]) + 0.999
            S[i, 0, 2] = np.floor(S[i, 0, 1]) + 0.5
        elif e == 5:
            S[i, 2, 0] = np.floor(abs(S[i, 2, 0])) + 1.0 + 1e-9
            S[i, 2, 1] = np.floor(S[i, 2, 0]) - 1e-9
            S[i, 3, 0] = np.floor(S[i, 2, 0])       # exactly the truncated neighbour
        elif e == 6:
            for k in (1, 2, 3):
                S[i, k, 0] = abs(S[i, 0, 0]) * (1 + 0.1 * k) + 1.0      # rising with b: negative ADC
        elif e == 7:
            s0 = abs(S[i, 0, 0]) + 10.0
            S[i, :, 0] = s0 * np.array([1.0, 0.5, 2e-2, 1e-3])          # ADC above 3
    return S.reshape(1, n, 4, 4)
