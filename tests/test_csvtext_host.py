"""The CSV text core (sequoia-pub_amd/csrc/fmt_core.h) built by the host compiler with the address and undefined-behaviour
sanitizers as a stand-alone program (tools/csvtext_hostcheck.cpp) and compared string for string with numpy and pandas:
float32 digits and layout over csvtext_cases.f32_bits() -- every exponent field, every power of two, the neighbours of every
power of ten: where shortest-digit routines part from one another (whether an interval bound counts as inside, the narrower
interval below a power of two); numpy counts a bound as inside for even mantissas only, and 4304 of these values print
differently with the bounds always excluded --, int64 text, and the rows of small frames against DataFrame.to_csv.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import csvtext_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    """The stand-alone program built with the host compiler and the sanitizers; run(mode, array bytes, *args) -> (stdout, bytes)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++ or clang++) to build tools/csvtext_hostcheck.cpp")
    build = tmp_path_factory.mktemp("csvtext_hostcheck")
    exe = str(build / "csvtext_hostcheck")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tools", "csvtext_hostcheck.cpp")], check=True)
    count = [0]

    def run(mode, data, *args):
        count[0] += 1
        src, dst = build / f"{count[0]}.in", build / f"{count[0]}.out"
        src.write_bytes(data)
        r = subprocess.run([exe, mode, str(src), str(dst), *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
        return r.stdout, dst.read_bytes()
    return run


def rows_file(df):
    index, ints, floats = cc.frame_parts(df)
    return np.array([len(df), ints.shape[1], floats.shape[1]], dtype=np.int64).tobytes() + index.tobytes() + ints.tobytes() + floats.tobytes()


def test_float32_text_equals_numpy_astype_str(hostcheck):
    bits, want = cc.f32_bits(), cc.f32_strings()
    assert len(bits) > 2_000_000 and len(want) == len(bits)
    _, out = hostcheck("f32", bits.tobytes())
    got = out.decode("ascii").split("\n")
    assert got.pop() == "" and len(got) == len(want)
    if got != want:
        bad = [(hex(int(b)), g, w) for b, g, w in zip(bits, got, want) if g != w]
        pytest.fail(f"{len(bad)} of {len(want)} float32 texts differ from numpy's; the first (bits, core, numpy): {bad[:10]}")
    assert max(map(len, got)) == 19


def test_float32_layout_examples(hostcheck):
    vals = np.array([1e-4, 1e-5, 3e16, 1e16, 9.999999e15, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -2.5, 0.1, 16777216.0, 1.17549435e-38, 1e-45,
                     3.4028235e38, 0.00012, 3333333500000000.0, -1e15], dtype=np.float32)
    want = ["1e-04", "1e-05", "3e+16", "1e+16", "9999999000000000.0", "0.0", "-0.0", "inf", "-inf", "", "1.0", "-2.5", "0.1", "16777216.0",
            "1.1754944e-38", "1e-45", "3.4028235e+38", "0.00012", "3333333500000000.0", "-1000000000000000.0"]
    assert [("" if np.isnan(v) else s) for v, s in zip(vals, vals.astype(str))] == want          # what numpy does, spelled out
    _, out = hostcheck("f32", vals.tobytes())
    assert out.decode("ascii").split("\n")[:-1] == want


def test_int64_text_equals_str(hostcheck):
    v = cc.i64_values()
    _, out = hostcheck("i64", v.tobytes())
    got = out.decode("ascii").split("\n")
    assert got[:-1] == [str(int(x)) for x in v] and max(map(len, got)) == 20


@pytest.mark.parametrize("name", list(cc.frames()))
def test_rows_equal_to_csv(hostcheck, name):
    df, _ = cc.frames()[name]
    want = df.to_csv(header=False).encode()
    assert df.iloc[:0].to_csv().encode() + want == df.to_csv().encode()                         # header and rows are separable
    stdout, out = hostcheck("rows", rows_file(df))
    assert out == want and f"{len(df)} rows, {len(want)} bytes, ok" in stdout


def test_front_end_host_logic():
    """What csvtext.py and the CLI decide without a device: the flag and its default, pandas' header from the empty frame, the
    frames the device writer does not take, and the chunk size that keeps a chunk's text inside the budget."""
    import pandas as pd
    from sequoia_pub_amd import csvtext
    from sequoia_pub_amd.cli import visualize
    parser = visualize.build_parser()
    assert parser.parse_args([]).table == "host" and parser.parse_args(["--table", "device"]).table == "device"
    with pytest.raises(SystemExit):
        parser.parse_args(["--table", "gpu"])
    for name, (df, _) in cc.frames().items():
        assert csvtext.header_line(df.columns, df.index) + df.to_csv(header=False).encode() == df.to_csv().encode(), name
    named = pd.DataFrame({"x": [1]}, index=pd.RangeIndex(1, name="tile"))
    assert csvtext.header_line(["x", "g"], named.index) == b"tile,x,g\n"
    ok = pd.DataFrame({"xcoord": np.arange(3), "ycoord": np.arange(3)})
    assert csvtext.frame_refusal(ok, ["G_0", "G"]) is None
    assert "int64" in csvtext.frame_refusal(ok.set_index(pd.Index(["a", "b", "c"])), ["G"])
    assert "xcoord (float64)" in csvtext.frame_refusal(ok.astype({"xcoord": float}), ["G"])
    assert "share a name" in csvtext.frame_refusal(ok, ["G", "xcoord"])
    assert csvtext.chunk_rows_for(4, 1536, 256 << 20) * (1 + 4 + 1536) * csvtext.MAX_CELL_BYTES <= 256 << 20
    assert csvtext.chunk_rows_for(4, 1536, 256 << 20) == (256 << 20) // (21 * 1541)
    assert csvtext.chunk_rows_for(0, 100000, 1 << 20) == 1                                        # a row beyond the budget: one row a chunk
    assert csvtext.chunk_rows_for(0, 0, 1 << 62) == csvtext.MAX_CELLS


def test_rows_stop_at_the_capacity(hostcheck):
    """The capacity rule of sq_csv_format_rows on the host: every byte below the capacity is the text's, the part of a cell
    that straddles it included, none is stored at or behind it (the program's buffer is exactly that long: a byte more is
    the sanitizer's to report) and the overflow is reported.  One byte short, in the middle of a cell, and 0."""
    df, _ = cc.frames()["ten_rows_chunk_3"]
    want = df.to_csv(header=False).encode()
    for capacity in (len(want) - 1, len(want) - 3, len(want) // 2, 1, 0):
        stdout, out = hostcheck("rows", rows_file(df), capacity)
        assert "overflow" in stdout and out == want[:capacity], capacity
    stdout, out = hostcheck("rows", rows_file(df), len(want))
    assert "ok" in stdout and out == want
