"""What tests/test_hip_grid_limits.py and tests/test_grid_limits_model.py share: batches of many lines whose expected values
cost the model 251 lines.

Where lines (rows, images, planes, bins) are independent of each other, line i of a batch is a copy of line i % P of P
distinct model lines, and the expected output is the model's output for those P lines, tiled the same way.  P = 251 is
prime and divides none of the launch-grid caps the batches exceed -- 16384, 65535 and 65536 leave 69, 24 and 25 -- so a
line fetched or stored one cap away from where it belongs meets different data.  A plain module like hipdev.py."""
import numpy as np

P = 251
CAPS = (16384, 65535, 65536)
assert all(c % P for c in CAPS)


def tile(a, n, axis=0):
    """n lines along `axis`, line i a copy of line i % a.shape[axis] of `a`"""
    a = np.asarray(a)
    return np.take(a, np.arange(n) % a.shape[axis], axis=axis)


def trips(n, cap):
    """how often the first workgroup of a loop `for (i = blockIdx; i < n; i += cap)` runs its body"""
    return -(-n // cap)


def oned(oracle, wv, inverse, lines, j_max):
    """the oracle's 1-D driver (tests/test_oned.py: restated) on every line of a float32 batch -> (batch, level count)"""
    from test_oned import restated

    out = np.array(lines, dtype=np.float32, copy=True)
    j = j_max
    for row in out:
        j = restated(oracle, wv, inverse, row, row.shape[0], None, j_max)
    return out, j
