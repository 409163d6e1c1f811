"""Cases of the device CSV text (sequoia_pub_amd.csvtext, csrc/csvtext.hip, csrc/fmt_core.h), shared by the host check
(tests/test_csvtext_host.py: the core built stand-alone under the sanitizers) and the device tests (tests/test_gpu_csvtext.py).
The references are numpy and pandas themselves: ``ndarray.astype(str)`` of float32 (NaN: the empty cell), ``str(int)`` and
``DataFrame.to_csv()``.  Each is computed once and must not be written to."""
import functools

import numpy as np
import pandas as pd

RANDOM_MANTISSAS = 4000
POWERS_OF_TEN = range(-45, 39)


@functools.lru_cache(maxsize=None)
def f32_bits():
    """uint32 bit patterns: every exponent field with the mantissas 0 (every power of two), 1, 2^23 - 2, 2^23 - 1 and
    RANDOM_MANTISSAS seeded random ones of its own, both signs (field 0: denormals and the zeros; field 255: the infinities
    and NaNs); every denormal power of two; the float32 at and 1, 2 ulp to either side of every power of ten 1e-45 .. 1e38
    (1e-4 and 1e16, where the layout changes, among them), both signs."""
    rs = np.random.RandomState(20261021)
    mant = np.concatenate([np.tile(np.array([0, 1, 2 ** 23 - 2, 2 ** 23 - 1], np.uint32), (256, 1)),
                           rs.randint(0, 2 ** 23, (256, RANDOM_MANTISSAS)).astype(np.uint32)], axis=1)
    fields = (np.arange(256, dtype=np.uint32) << 23)[:, None] | mant
    tens = np.array([float(f"1e{k}") for k in POWERS_OF_TEN], dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.int64)
    near = (tens[:, None] + np.arange(-2, 3)[None, :]).ravel()
    near = near[(near >= 0) & (near < 0x7F800000)].astype(np.uint32)
    pos = np.concatenate([fields.ravel(), np.uint32(1) << np.arange(23, dtype=np.uint32), near])
    bits = np.concatenate([pos, pos | np.uint32(0x80000000)])
    bits.setflags(write=False)
    return bits


@functools.lru_cache(maxsize=None)
def f32_strings():
    """numpy's text of every f32_bits() value, NaN as the empty cell (to_csv's na_rep): a list of str."""
    vals = f32_bits().view(np.float32)
    text = vals.astype(str)
    return np.where(np.isnan(vals), "", text).tolist()


def i64_values():
    """0, +-1, +-(10^k - 1), +-10^k for every k an int64 holds, the extremes."""
    v = [0, 1, -1, np.iinfo(np.int64).min, np.iinfo(np.int64).max]
    for k in range(1, 19):
        v += [10 ** k, -(10 ** k), 10 ** k - 1, -(10 ** k - 1)]
    return np.array(v, dtype=np.int64)


def _floats(rs, shape):
    """float32 values over many magnitudes, some integers, zeros of both signs and infinities among them."""
    a = (rs.randn(*shape) * np.exp(rs.randn(*shape) * 6)).astype(np.float32)
    pick = rs.rand(*shape)
    a[pick < 0.10] = np.round(a[pick < 0.10])
    a[(pick >= 0.10) & (pick < 0.12)] = 0.0
    a[(pick >= 0.12) & (pick < 0.14)] = -0.0
    a[(pick >= 0.14) & (pick < 0.15)] = np.inf
    a[(pick >= 0.15) & (pick < 0.16)] = -np.inf
    a[(pick >= 0.16) & (pick < 0.22)] = np.nan
    return a


def _frame(rs, n, ints, floats, start=0, int_scale=1000):
    cols = {}
    for name in ints:
        cols[name] = (rs.randint(-int_scale, int_scale, n)).astype(np.int64)
    data = _floats(rs, (n, len(floats)))
    for k, name in enumerate(floats):
        cols[name] = data[:, k]
    return pd.DataFrame(cols, index=pd.RangeIndex(start, start + n), columns=list(ints) + list(floats))


@functools.lru_cache(maxsize=None)
def frames():
    """name -> (DataFrame with a RangeIndex, int64 columns then float32 columns; rows per chunk or None for one chunk)."""
    rs = np.random.RandomState(7)
    out = {}
    out["no_rows"] = (_frame(rs, 0, ["xcoord", "ycoord"], ["G1_0", "G1"]), None)
    out["one_cell"] = (_frame(rs, 1, [], ["G"]), None)
    out["ten_rows_chunk_3"] = (_frame(rs, 10, ["xcoord", "ycoord", "xcoord_tf", "ycoord_tf"], ["A_0", "A_1", "A"]), 3)
    third = _frame(rs, 31, ["x"], ["a", "b", "c", "d"])
    third.iloc[::3, 1:] = np.nan
    out["every_third_row_nan"] = (third.astype({c: np.float32 for c in "abcd"}), 7)
    out["one_row_5000_columns"] = (_frame(rs, 1, ["x"], [f"g{i}" for i in range(5000)]), None)
    out["4097_rows_one_column"] = (_frame(rs, 4097, [], ["g"]), None)
    big = _frame(rs, 9, ["a", "b"], ["v"])
    big["a"] = np.array([0, -1, 1, np.iinfo(np.int64).min, np.iinfo(np.int64).max, 10 ** 18, -(10 ** 18), 999, -1000], dtype=np.int64)
    big["b"] = -big["a"].values[::-1].copy()
    out["negative_and_large_ints"] = (big, 4)
    out["index_from_123456"] = (_frame(rs, 12, ["x", "y"], ["quoted, name", "g"], start=123456), 5)
    for name, (df, _) in out.items():
        kinds = [str(t) for t in df.dtypes]
        assert kinds == sorted(kinds, key=lambda s: s != "int64") and set(kinds) <= {"int64", "float32"}, (name, kinds)
    return out


def frame_parts(df):
    """(index int64 [n], ints int64 [n, n_int], floats float32 [n, n_f32]) of a case frame, C-contiguous."""
    ints = [c for c in df.columns if df[c].dtype == np.int64]
    floats = [c for c in df.columns if df[c].dtype == np.float32]
    n = len(df)
    return (np.ascontiguousarray(df.index.values, dtype=np.int64),
            np.ascontiguousarray(df[ints].values, dtype=np.int64).reshape(n, len(ints)),
            np.ascontiguousarray(df[floats].values, dtype=np.float32).reshape(n, len(floats)))


def fold_tables(F, n=1000, cols=7, seed=11):
    """float32 [F, n, cols]: seeded values with scattered NaNs, zeros of both signs, rows that are NaN in every fold and
    rows with one value."""
    rs = np.random.RandomState(seed + F)
    a = (rs.randn(F, n, cols) * np.exp(rs.randn(F, n, cols) * 3)).astype(np.float32)
    pick = rs.rand(F, n, cols)
    a[pick < 0.2] = np.nan
    a[(pick >= 0.2) & (pick < 0.25)] = -0.0
    a[(pick >= 0.25) & (pick < 0.27)] = 0.0
    a[:, 5::50, :] = np.nan
    a[1:, 7::50, :] = np.nan
    return a


def pandas_fold_mean(a):
    """DataFrame.mean(axis=1) per column group, as cli.visualize computes the fold mean: float32 [n, cols]."""
    F, n, cols = a.shape
    out = np.empty((n, cols), dtype=np.float32)
    for c in range(cols):
        fr = pd.DataFrame({f"g_{f}": a[f, :, c] for f in range(F)})
        m = fr[[f"g_{f}" for f in range(F)]].mean(axis=1)
        assert m.dtype == np.float32
        out[:, c] = m.values
    return out
