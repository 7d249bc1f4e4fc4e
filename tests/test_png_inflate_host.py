"""The device PNG reader's inflate (csrc/nic_inflate.h) on the CPU, at deflate's edges: the edge streams
of tests/png_read_cases.py -- hand-written deflate that is legal but that zlib never writes, and one
defect each for the refused ones -- are judged by zlib (an implementation that is not ours), each
accepted one proves on png_parse.deflate_blocks' report that it reaches the edge it is named for, and
tools/png_read_host_check.cpp is built as the stand-alone program it is, under AddressSanitizer and
UBSan where they link, and run over the whole corpus: exact statuses, and output bytes equal to
zlib's.  tests/test_gpu_png_read.py then repeats on the GPU what the CPU has agreed to here."""
import importlib.util
import os
import re
import shutil
import subprocess
import zlib

import pytest

from tests import png_parse, png_read_cases as C

ROOT = C.ROOT
E = C.edge_streams


def T_of(shape) -> int:
    h, w, ch = shape
    return h * (w * ch + 1)


def blocks(name):
    stream, _, status = E()[name]
    assert status == 0
    return png_parse.deflate_blocks(stream, trailing=name == "bytes_after_adler")


ACCEPTED = sorted(n for n, v in E().items() if v[2] == 0)
REFUSED = sorted(n for n, v in E().items() if v[2] != 0)


def test_the_case_table_by_status():
    st = {n: v[2] for n, v in E().items()}
    assert len(ACCEPTED) == 50 and len(REFUSED) == 27
    assert sorted(n for n in REFUSED if st[n] == 1) == ["cinfo_8", "cm_7", "empty_stream", "fcheck_off_by_one", "fdict", "one_byte_stream"]
    assert sorted(n for n in REFUSED if st[n] == 4) == ["match_passes_T", "stored_passes_T", "three_adler_bytes"]
    assert all(st[n] == 2 for n in REFUSED if st[n] not in (1, 4)) and sum(st[n] == 2 for n in REFUSED) == 18
    assert len(E()["one_byte_stream"][0]) == 1 and len(E()["empty_stream"][0]) == 0


@pytest.mark.parametrize("name", sorted(E()))
def test_zlib_is_the_judge(name):
    """zlib.decompress returns exactly T bytes iff the expected status is 0."""
    stream, shape, status = E()[name]
    try:
        n = len(zlib.decompress(stream))
    except zlib.error:
        n = None
    assert (n == T_of(shape)) == (status == 0), (n, T_of(shape), status)


@pytest.mark.parametrize("name", ACCEPTED)
def test_filter_bytes_are_zero(name):
    C.edge_image(name)  # asserts it


# ---- each accepted case reaches its edge ----------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in ACCEPTED if n.startswith("far_")])
def test_far_cases_hold_the_one_match_they_are_named_for(name):
    b = blocks(name)
    assert [x["type"] for x in b] == ["stored", "fixed", "stored"] and b[1]["matches"] == 1 and b[1]["symbols"] == 1
    (at, length, dist), = b[1]["far"]
    want = {"far_wrap_32668_at_dist": (32668, 258, 32668), "far_wrap_32511": (32668, 258, 32511), "far_32768_len3": (33000, 3, 32768),
            "far_32768_len130": (32900, 130, 32768), "far_32768_sym284": (33000, 258, 32768)}
    if name in want:
        assert (at, length, dist) == want[name]
    else:
        _, d, _, where = name.split("_")
        assert (length, dist) == (258, int(d)) and at == (dist if where == "dist" else 33000)
    assert at == b[1]["out_start"] and dist == b[1]["max_dist"] and b[1]["reach"] == dist
    assert dist >= 32506  # zlib's own farthest, and beyond
    assert b[1]["len_symbols"] == ({284} if name.endswith("sym284") else {285 if length == 258 else 257 if length == 3 else 280})
    if "wrap" in name:
        assert (at & 32767) == 32768 - 100 and (at & 32767) + length > 32768  # the destination wraps the ring's end
    # the block before the final stored one ends mid-byte (but for length 130, whose fixed block is 40 bits)
    assert (b[2]["start_bit"] % 8 != 0) == (length != 130)
    assert b[1]["out_start"] + length == b[2]["out_start"] and b[2]["out_start"] + b[2]["symbols"] == T_of(C.FAR_SHAPE)


def test_far_cases_cover_every_distance_from_the_ring_s_size_down_to_zlib_s_farthest():
    names = {n for n in ACCEPTED if n.startswith("far_")}
    for d in (32768, 32767, 32705, 32704, 32511, 32510, 32506):
        assert {f"far_{d}_at_dist", f"far_{d}_at_33000"} <= names
    assert C.FAR_DISTANCES == (32768, 32767, 32705, 32704, 32511, 32510, 32506)


def test_long_literal_codes_are_decoded():
    b, = blocks("long_lit_codes")
    assert b["type"] == "dynamic" and sorted(l for l in b["lit_lens"] if l) == C.LONG_LENS  # every length 1..15, complete
    assert sum(2.0 ** -l for l in b["lit_lens"] if l) == 1.0
    assert b["used_lens"] == set(range(1, 16)) and b["used_len"] == 15 and b["max_len"] == 15
    assert all(b["lit_lens"][v] == v + 1 for v in range(10, 15))  # literals at 11, 12, 13, 14 and 15 bits
    assert set(range(10, 15)) <= set(zlib.decompress(E()["long_lit_codes"][0]))


def test_long_distance_codes_are_decoded():
    b, = blocks("long_dist_codes")
    assert sorted(l for l in b["dist_lens"] if l) == C.LONG_LENS and sum(2.0 ** -l for l in b["dist_lens"]) == 1.0
    assert b["dist_used_lens"] >= {11, 12, 13, 14, 15} and b["dist_used_len"] == 15 and b["dist_max_len"] == 15
    assert b["matches"] == 6 and b["used_len"] == 15 and b["lit_lens"][257] == 15  # the length symbol is a 15-bit code too


def test_code_16_and_18_cross_the_hlit_boundary():
    b, = blocks("code16_across_hlit")
    (s, rep, at), = [c for c in b["cl_symbols"] if c[0] == 16]
    assert at < b["hlit"] < at + rep and (at, rep) == (257, 6)
    assert b["lit_lens"][257] == 3 and b["dist_lens"] == [3] * 8 and b["matches"] == 2
    b, = blocks("code18_across_hlit")
    s, rep, at = [c for c in b["cl_symbols"] if c[0] == 18][-1]
    assert at < b["hlit"] < at + rep and (b["hlit"], at, rep) == (270, 257, 18)
    assert b["dist_lens"] == [0] * 5 + [1, 1]


def test_hclen_hlit_and_hdist_forms():
    b, = blocks("hclen_5")  # HCLEN 4 cannot be accepted: it allows only the lengths 0, so no end-of-block code
    assert b["hclen"] == 5 and set(b["lit_lens"]) == {0, 8}
    b, = blocks("hclen_19")
    assert b["hclen"] == 19 and b["cl_lens"][15] != 0 and 15 in b["lit_lens"]
    b, = blocks("hlit_257_hdist_1")
    assert (b["hlit"], b["hdist"], b["dist_lens"], b["matches"]) == (257, 1, [1], 0)
    b, = blocks("one_code_distance_set")
    assert b["dist_lens"] == [1] and b["matches"] == 4 and b["dist_used_lens"] == {1} and b["max_dist"] == 1
    b, = blocks("empty_distance_set")
    assert b["dist_lens"] == [0] and b["dist_max_len"] == 0 and b["matches"] == 0 and b["symbols"] == 4096


def test_flushes_and_block_sequences():
    b = blocks("sync_and_full_flush")
    empty = [k for k, x in enumerate(b) if x["type"] == "stored" and x["symbols"] == 0 and not x["final"]]
    assert len(empty) == 2 and b[empty[0]]["out_start"] == 2048 and b[empty[1]]["out_start"] == 3072
    after = b[empty[0] + 1]
    assert after["out_start"] == 2048 and after["matches"] > 0 and after["reach"] > 0 and after["max_dist"] == 2048
    assert all(x["reach"] <= 0 for x in b[empty[1] + 1:] if x["type"] != "stored")  # a full flush forgets the window
    b = blocks("twelve_blocks")
    assert [x["type"] for x in b] == ["stored", "fixed", "dynamic"] * 4
    assert all(x["matches"] == 1 and x["reach"] == 315 for x in b if x["type"] != "stored")  # into the block before
    assert any(x["start_bit"] % 8 for x in b if x["type"] == "stored")  # a stored block after one that ends mid-byte
    b = blocks("stored_65535_then_0")
    assert [(x["type"], x["symbols"], x["final"]) for x in b] == [("stored", 65535, 0), ("stored", 0, 1)]
    b = blocks("bytes_after_adler")
    assert len(E()["bytes_after_adler"][0]) == 2 + 5 + 4096 + 4 + 5
    with pytest.raises(AssertionError, match="bytes between"):
        png_parse.deflate_blocks(E()["bytes_after_adler"][0])


@pytest.mark.parametrize("p", C.RESTAGE_BYTES)
def test_headers_sit_on_the_input_ring_s_first_restage(p):
    b = blocks(f"block_header_at_{p}")
    assert [x["type"] for x in b] == ["stored", "fixed"] and b[1]["start_bit"] == 8 * p
    b = blocks(f"stored_len_at_{p}")
    assert [x["type"] for x in b] == ["stored", "stored"] and b[1]["start_bit"] == 8 * (p - 1) and b[1]["data_byte"] == p + 4
    assert C.RESTAGE_BYTES == tuple(range(2040, 2049))


def test_the_walker_reports_what_zlib_wrote():
    """The two streams of test_gpu_png_read.py::test_far_window_and_small_window, which the walker could
    not walk while it dropped every distance code's bits."""
    import numpy as np

    from tests import png_make as M

    top = C.rgb_image(64, 96)
    a = np.ascontiguousarray(np.concatenate([top, top]))
    far = png_parse.deflate_blocks(png_parse.parse(M.make_png(a, 0, level=9)).idat)
    near = png_parse.deflate_blocks(png_parse.parse(M.make_png(a, 0, level=9, wbits=9)).idat)
    assert max(b["max_dist"] for b in far) == 18496 and max(b["max_dist"] for b in near) <= 512 - 262


# ---- the host check, built and run --------------------------------------------------------------
def _corpus_module():
    spec = importlib.util.spec_from_file_location("png_read_corpus", os.path.join(ROOT, "tools", "png_read_corpus.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_host_check_over_the_extended_corpus(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler: tools/png_read_host_check.cpp was not built")
    exe, src = str(tmp_path / "png_read_host_check"), os.path.join(ROOT, "tools", "png_read_host_check.cpp")
    base = [cxx, "-std=c++17", "-O1", "-g", src, "-o", exe]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if sanitized.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr
    n, taken, pinned = _corpus_module().write(str(tmp_path / "corpus"))
    assert n >= 4156 + len(E()) and pinned >= 19 + len(E()) and taken >= 10 + len(ACCEPTED)
    run = subprocess.run([exe, str(tmp_path / "corpus")], capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    m = re.search(r"^(\d+) streams: .* (\d+) outputs compared with zlib's bytes; (\d+) exact statuses; 0 failures$", run.stdout, re.M)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (n, taken, pinned), run.stdout[-500:]
    if sanitized.returncode != 0:
        pytest.skip("the host check passed (0 failures), but WITHOUT sanitizers: their runtimes do not link here: "
                    + sanitized.stderr.strip()[-300:])
