"""The first block of a band without the dead stages of the pipeline fill (k_iterate_tbr, step_r FILLB) and bands of any height.

A band wave's first block skips every stage whose output no stored value depends on (stage t while step <= 2t), and the planner may
cut bands whose height leaves any residue of (rows + 2T) mod P.  Both must be invisible: for every fixed-work block length of the
tables -- independent waves 10, 8, 6, 5, 4, 3, 2, 1; the joined waves (T = 10) with and without a |grad|^2 plane; the illumination
channel's 10, 5, 2, 1; the exact-math blocks 5 .. 1 -- two passes of the block with the band height forced to 13 consecutive values
(every residue mod P for every P <= 13) and to more than the image height (one band), with p read and with the first pass's p = 0
form: u AND p equal, array for array, to one launch per iteration (blocks of 1 on independent waves; the one-iteration exact kernel
for exact math) and to the register tiles, whose kernel has no pipeline.

Not covered: poisoned rows outside the image -- the stage entry copies the caller's planes into dense scratch planes of exactly the
image's rows, and the kernels clamp their row addresses into them, so there is no such row to poison.
"""
import numpy as np
import pytest

from test_tvl1_stage_kernels import GAMMA, _assert_same, _inputs, _run

pytestmark = pytest.mark.gpu

SHAPES = [(157, 301), (61, 777)]   # odd sizes; 777 columns: four strips of joined waves, all four waves live, a ragged last group
ROWS = list(range(8, 21))          # 13 consecutive band heights


def _band_heights(h):
    return ROWS + [h + 5]


def _reference(gpu, x, niter, cache, **kw):
    """One launch per iteration: blocks of 1 (cached per iteration count and p = 0 form)."""
    key = (niter, bool(kw.get("p_zero")), kw.get("gamma", 0.0))
    if key not in cache:
        form = "blocked" if kw.get("gamma", 0.0) != 0.0 else "indep"   # (the channel's T = 1 kernel runs independent waves)
        cache[key] = _run(gpu, form, x, niter, blocks=[1] * niter, **kw)[0]
    return cache[key]


@pytest.mark.parametrize("shape", SHAPES)
def test_independent_wave_blocks_equal_one_launch_per_iteration(gpu, shape):
    x = _inputs(*shape, seed=41)
    cache = {}
    for T in (10, 8, 6, 5, 4, 3, 2, 1):
        for pz in (False, True):
            ref = _reference(gpu, x, 2 * T, cache, p_zero=pz)
            tile = _run(gpu, "tile", x, 2 * T, blocks=[T, T], p_zero=pz)[0]
            _assert_same(tile, ref, False, f"register tiles T={T} p_zero={pz} vs one launch per iteration")
            for rows in _band_heights(shape[0]):
                got, _ = _run(gpu, "indep", x, 2 * T, blocks=[T, T], rows_per_band=rows, p_zero=pz)
                _assert_same(got, ref, False, f"independent waves T={T} rows_per_band={rows} p_zero={pz}")


@pytest.mark.parametrize("shape", SHAPES)
def test_joined_wave_blocks_equal_one_launch_per_iteration(gpu, shape):
    """The kernels of record: T = 10 joined waves forming |grad|^2 themselves (what calc() runs) and reading the plane."""
    x = _inputs(*shape, seed=43)
    cache = {}
    for pz in (False, True):
        for niter in (10, 20):
            ref = _reference(gpu, x, niter, cache, p_zero=pz)
            for rows in _band_heights(shape[0]):
                for ng in (True, False):
                    got, _ = _run(gpu, "blocked", x, niter, nograd=ng, time_block=10, rows_per_band=rows, p_zero=pz)
                    _assert_same(got, ref, False, f"joined waves NG={ng} niter={niter} rows_per_band={rows} p_zero={pz}")
    # mixed passes as calc() decomposes other iteration counts (joined 10 + independent 6 / 1), planner's band height and forced ones
    ref = _reference(gpu, x, 17, cache)
    for rows in (0, 9, 16):
        got, _ = _run(gpu, "blocked", x, 17, blocks=[10, 6, 1], rows_per_band=rows)
        _assert_same(got, ref, False, f"blocks [10, 6, 1] rows_per_band={rows}")


@pytest.mark.parametrize("shape", SHAPES)
def test_gamma_blocks_equal_one_launch_per_iteration(gpu, shape):
    x = _inputs(*shape, seed=47, gam=True)
    cache = {}
    for T in (10, 5, 2, 1):
        for pz in (False, True):
            ref = _reference(gpu, x, 2 * T, cache, p_zero=pz, gamma=GAMMA)
            if T == 10:
                tile = _run(gpu, "tile", x, 2 * T, blocks=[T, T], p_zero=pz, gamma=GAMMA, variant=0)[0]
                _assert_same(tile, ref, True, f"register tiles, gamma, p_zero={pz} vs one launch per iteration")
            for rows in _band_heights(shape[0]):
                got, _ = _run(gpu, "blocked", x, 2 * T, blocks=[T, T], rows_per_band=rows, p_zero=pz, gamma=GAMMA)
                _assert_same(got, ref, True, f"gamma T={T} rows_per_band={rows} p_zero={pz}")


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_blocks_equal_the_one_iteration_exact_kernel(gpu, shape):
    x = _inputs(*shape, seed=53)
    for T in (5, 4, 3, 2, 1):
        for pz in (False, True):
            ref, _ = _run(gpu, "one", x, 2 * T, exact=True, p_zero=pz)
            for rows in _band_heights(shape[0]):
                got, _ = _run(gpu, "exact_blocked", x, 2 * T, blocks=[T, T], rows_per_band=rows, p_zero=pz)
                _assert_same(got, ref, False, f"exact T={T} rows_per_band={rows} p_zero={pz}")
