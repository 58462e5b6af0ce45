"""GPU: batch_normalize (fvdb_batch_normalize; src/core/vector_ops.rs:138-150) bit for bit against tests/_cos_ref.py."""
import numpy as np
import pytest

import fvdb_import
import _cos_ref as ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", [1, 33, 384])
def test_batch_normalize_bits(d):
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    rng = np.random.default_rng(d)
    x = rng.standard_normal((301, d)).astype(np.float32)  # more than one workgroup, a partial last one
    x *= np.exp2(rng.integers(-30, 31, 301)).astype(np.float32)[:, None]
    x[7] = 0  # a zero row is returned unchanged
    x[8] = -0.0
    got = fv.batch_normalize(ctx, x)
    assert np.array_equal(got.view(np.uint32), ref.normalize(x).view(np.uint32))
    assert np.array_equal(got[7:9].view(np.uint32), x[7:9].view(np.uint32))
    ctx.close()
