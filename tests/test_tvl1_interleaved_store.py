"""The calc's final pass writes the callers' CV_32FC2 matrices itself (k_iterate_tbr, TbArgs::otab) instead of u planes + k_pack_flow.

A batch of four pairs of 1283 x 961 (two lanes of two pairs: level 0 is a streaming level, its last pass stores interleaved) into
output matrices of a padded pitch, against the same pairs computed one per calc() -- a single pair of this size iterates on the
register tiles and goes through k_pack_flow: flows equal bit for bit, and not one byte of the pitch padding touched.  f32 and u8
input; 10 iterations (one T = 10 pass per warp) and 7 (passes of 6 + 1: a last block that is not T = 10, on independent waves).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, N = 961, 1283, 4
PAD = 37            # pixels (of two floats) of pitch padding behind every row
SENTINEL = -12345.5


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("iterations", [10, 7])
def test_batch_into_pitched_matrices_equals_single_calcs(gpu, dtype, iterations):
    import torch
    from opencv_contrib_amd import cuda, synth
    pairs = [synth.flow_pair(H, W, seed=60 + b, **({"dtype": "u8"} if dtype == "u8" else {}))[:2] for b in range(N)]
    I0 = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a, _ in pairs]
    I1 = [torch.from_numpy(np.ascontiguousarray(b)).to(gpu) for _, b in pairs]
    kw = dict(iterations=iterations, epsilon=0.0)
    singles = [cuda.OpticalFlowDual_TVL1.create(**kw).calc(a, b).cpu().numpy() for a, b in zip(I0, I1)]
    backing = torch.full((N, H, W + PAD, 2), SENTINEL, dtype=torch.float32, device=gpu)
    flows = [backing[b, :, :W, :] for b in range(N)]
    assert flows[0].stride(0) == 2 * (W + PAD)
    alg = cuda.OpticalFlowDual_TVL1.create(**kw)
    for _ in range(2):   # a second call on the same handle: cached plan, arena and pointer table
        alg.calc_batch(I0, I1, flows)
        torch.cuda.synchronize()
        out = backing.cpu().numpy()
        assert (out[:, :, W:, :] == np.float32(SENTINEL)).all(), "pitch padding written"
        for b in range(N):
            assert np.isfinite(out[b, :, :W, :]).all()
            np.testing.assert_array_equal(out[b, :, :W, :], singles[b], err_msg=f"pair {b} {dtype} N={iterations}")
        backing[:, :, :W, :] = 0.0
