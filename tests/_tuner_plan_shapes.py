"""The shapes tests/test_gpu_tuner_plans.py runs, each with the plan it was chosen for: which of the wideband tuner's matrix
kernels takes the call (tiles per wave and step), whether a step's outputs go through the LDS buffer or are stored piece by
piece, how many workgroups share a CU, the LDS, and how many steps a workgroup walks.  The figures are those
tests/cpp/tuner_plan_check.cpp prints from the product's host arithmetic (csrc/tuner_host.hpp); tests/test_tuner_plan_host.py
holds every row against that program on the CPU, and the GPU tests hold Tuner.plan() against the row before they compare a
byte, so a changed limit cannot move a case off the path it is there for without a test saying so.

A shape is (U, D, T, fmt): rate U / D (U = 1, D <= 32: the integer kernels), T taps of the prototype, input format."""
from math import gcd

U8, S8, S16 = 0, 1, 2                 # _tuner_formats_model's, FMRX_TUNER_*
TWO_PER_CU, ONE_PER_CU = 65536, 163840   # LDS limits of a workgroup (kTwoPerCu, kOnePerCu)


def plan_row(U, D, T, fmt, tiles, via_lds, per_cu, lds_bytes=None, N=5, n_wide=None, n_steps=None, steps_per_wg=None, grid=None):
    return dict(U=U, D=D, T=T, fmt=fmt, tiles=tiles, via_lds=via_lds, per_cu=per_cu, lds_bytes=lds_bytes, N=N,
                n_wide=D if n_wide is None else n_wide, n_steps=n_steps, steps_per_wg=steps_per_wg, grid=grid)


def row_id(r):
    return f"{r['U']}_{r['D']}_T{r['T']}_{('u8', 's8', 's16')[r['fmt']]}_N{r['N']}"


# C1: a workgroup that walks three steps, the last one of the call ragged.  4099 = 2 * 2048 + 3 steps on one row of workgroups
# (N = 3: one channel group, one lane group idle) -> 3 steps per workgroup, the last workgroup a single, partial step.  The call
# is the 4099 steps' outputs less 5 (integer rates) or less 3 periods of U outputs (rational ones).
def _steps_row(U, D, T, fmt, tiles, via_lds, lds):
    step_out = 128 * U * tiles
    n_out = 4099 * step_out - (5 if U == 1 else 3 * U)
    return plan_row(U, D, T, fmt, tiles, via_lds, 2, lds, N=3, n_wide=n_out // U * D, n_steps=4099, steps_per_wg=3, grid=(1367, 1))


MULTI_STEP = [
    _steps_row(1, 4, 9, U8, 4, False, 21680),
    _steps_row(1, 4, 9, S8, 4, False, 21680),
    _steps_row(1, 4, 9, S16, 2, False, 21856),
    _steps_row(2, 5, 9, U8, 4, True, 55456),
    _steps_row(2, 5, 9, S8, 4, True, 55456),
    _steps_row(2, 5, 9, S16, 2, True, 39232),
    _steps_row(6, 13, 9, U8, 1, True, 44832),       # the smallest D at which U = 6 plans one tile at any T
    _steps_row(5, 11, 9, S16, 1, True, 43456),
]
# the steps spread over five rows of workgroups: 70 channels, 820 steps of 256 outputs less 5 -> 3 steps per workgroup, 274 x 5
MULTI_STEP_ROWS = plan_row(1, 4, 9, S16, 2, False, 2, 21856, N=70, n_wide=4 * (820 * 256 - 5), n_steps=820, steps_per_wg=3, grid=(274, 5))

# C2: every plan class of the rational kernels at its edge (tuner_plan_check's `largest` and `smallest` shapes, the two sides of
# the flip to direct stores at 20/119, and the largest LDS the plan accepts at all)
PLAN_CLASSES = [
    plan_row(20, 121, 2, S16, 1, False, 1, 82880),       # direct stores: the smallest shape
    plan_row(21, 125, 3886, S16, 1, False, 1, 85824),    # direct stores: the largest LDS
    plan_row(20, 119, 820, S16, 1, True, 1, 163776),     # the last T of 20/119 that keeps the buffer ...
    plan_row(20, 119, 821, S16, 1, False, 1, 81984),     # ... and the first that stores directly
    plan_row(20, 119, 181, S16, 1, True, 1, 163776),     # the largest LDS of all: 64 bytes under 160 KiB
    plan_row(24, 125, 3673, U8, 1, True, 1, 149344),     # the 8-bit formats' largest
    plan_row(10, 27, 2331, U8, 1, True, 2, 65520),       # 16 bytes under the two-per-CU limit, by tiles
    plan_row(4, 29, 869, U8, 2, True, 2, 65520),
    plan_row(2, 13, 499, S8, 4, True, 2, 64320),
    plan_row(8, 27, 1865, S16, 1, True, 2, 65504),
    plan_row(2, 29, 451, S16, 2, True, 2, 65504),
]


def class_periods(r):
    """calls of D times these wide samples: one period, a partial piece, a partial tile, and more than one step (a step is
    128 periods per tile: 300 periods cross one at 1 and 2 tiles, the 4-tile kernels need 549)"""
    return (1, 3, 40, max(300, 128 * r["tiles"] + 37))


DIRECT_17_CHANNELS = plan_row(20, 121, 2, S16, 1, False, 1, 82880, N=17)     # the second row of workgroups holds one channel
DIRECT_PITCH = plan_row(20, 119, 821, S16, 1, False, 1, 81984, N=5)          # into a pitch larger than the row


# C3: rates.  Integer: every R with T in {2, 2 R + 1, 256}; the plan is fixed (4 tiles, 2 for S16, direct stores).
INTEGER_RATES = list(range(2, 33))


def integer_taps(R):
    return (2, 2 * R + 1, 256)


def integer_row(R, T, fmt, N=7):
    return plan_row(1, R, T, fmt, 2 if fmt == S16 else 4, False, 2, N=N)


def coprime_from(U, D, step):
    while gcd(U, D) != 1:
        D += step
    return D


def rational_rates():
    """(U, D): prime U, the top of the range and its neighbour, each at D = 2 U + 1, a middle D and the largest coprime D <= 125"""
    out = []
    for U in (5, 7, 23, 24):
        lo = 2 * U + 1
        hi = coprime_from(U, 125, -1)
        out += [(U, lo), (U, coprime_from(U, (lo + hi) // 2, 1)), (U, hi)]
    return out


def rational_taps(U, D):
    return (U + 1, 8 * D)


# every count of stored K-steps per image (ksp = 1 .. 9), for the integer and for the rational kernels: tuner_plan_check's first
# shape of each, as {ksp: (U, D, T)}
KSP_INTEGER = {1: (1, 2, 2), 2: (1, 2, 18), 3: (1, 2, 50), 4: (1, 2, 82), 5: (1, 2, 114), 6: (1, 2, 146), 7: (1, 2, 178), 8: (1, 2, 210),
               9: (1, 2, 242)}
KSP_RATIONAL = {1: (2, 5, 2), 2: (2, 5, 5), 3: (2, 5, 69), 4: (2, 5, 133), 5: (2, 5, 197), 6: (2, 5, 261), 7: (2, 5, 325), 8: (2, 5, 389),
                9: (2, 5, 453)}
# 16 and 17 channels: the last channel group of a row of workgroups full, and a second row for one channel
SIXTEEN_SEVENTEEN = [(1, 3, 7), (7, 15, 8)]
