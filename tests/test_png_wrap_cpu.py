"""The device CRC-32 and PNG / APNG assembly, the parts that need no GPU: the entry points are declared, bound and exported;
the size functions are what the header derives and what write_apng's layout implies; bad arguments are refused on the host,
before anything is launched (every call here must fail in the checks: its pointers point nowhere)."""

import os
import re

from tests import png_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sp_crc32_ws_bytes", "sp_crc32_rows", "sp_png_file_bytes", "sp_apng_file_bytes", "sp_png_wrap_ws_bytes", "sp_png_wrap")


def test_new_symbols_are_declared_bound_and_exported():
    from vdpp_amd import hip
    header = open(os.path.join(ROOT, "include", "svdpipe.h")).read()
    declared = set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", header))
    lib = hip.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/svdpipe.h"
        assert name in hip.SIGNATURES, f"{name} is not in the ctypes table"
        assert hasattr(lib, name), f"{name} is not exported"
    assert len(hip.SIGNATURES["sp_png_wrap"][1]) == 15 and len(hip.SIGNATURES["sp_crc32_rows"][1]) == 9


def test_size_functions_are_the_layouts_sums():
    from vdpp_amd.hip import ops
    from vdpp_amd.models.image_io import png_file, write_apng
    for h, w, rows in ((576, 1024, 16), (50, 37, 3), (1, 1, 1), (64, 128, 100)):
        bound = pm.stream_bound(h, w, rows)
        assert ops.png_stream_bytes(h, w, rows) == bound
        assert ops.png_file_bytes(h, w, rows) == bound + 57
        for n in (1, 2, 14):
            assert ops.apng_file_bytes(n, h, w, rows) == 65 + n * (50 + bound) + 4 * (n - 1)
    # the same sums from the host's files of streams of a given length
    for n, size in ((1, 0), (1, 9), (3, 100), (14, 1000)):
        streams = [bytes(size)] * n
        assert len(png_file(7, 5, streams[0])) == size + 57
        assert len(write_apng(None, streams, 5, 7, 7)) == 65 + n * (50 + size) + 4 * (n - 1)
    for h, w, rows in ((0, 8, 1), (8, 0, 1), (65536, 1, 1), (4097, 4096, 16), (8, 8, 0)):
        assert ops.png_file_bytes(h, w, rows) == 0 and ops.apng_file_bytes(2, h, w, rows) == 0
    assert ops.apng_file_bytes(0, 8, 8, 1) == 0 and ops.apng_file_bytes(-1, 8, 8, 1) == 0
    assert ops.crc32_ws_bytes(14, 16384) == 4 * 14 and ops.crc32_ws_bytes(14, 16385) == 4 * 14 * 2
    assert ops.crc32_ws_bytes(0, 100) == 0 and ops.crc32_ws_bytes(1, 0) == 0
    assert ops.png_wrap_ws_bytes(14, 16385) == 256 + 4 * 14 * 2 and ops.png_wrap_ws_bytes(17, 100) == 512 + 4 * 17
    assert ops.png_wrap_ws_bytes(0, 100) == 0 and ops.png_wrap_ws_bytes(3, 0) == 0


def test_bad_arguments_are_refused_without_a_launch():
    from vdpp_amd import hip
    lib = hip.load()
    p = 0x10000                                  # never dereferenced: the checks come first
    cap, n = 1000, 3
    ws = lib.sp_png_wrap_ws_bytes(n, cap)
    still, movie = cap + 57, 65 + n * (50 + cap) + 4 * (n - 1)

    def wrap(streams=p, cap=cap, lens=p, n=n, h=16, w=32, animate=0, num=1, den=7, files=p, file_cap=still, file_len=p, ws_ptr=p,
             ws_bytes=ws):
        return lib.sp_png_wrap(streams, cap, lens, n, h, w, animate, num, den, files, file_cap, file_len, ws_ptr, ws_bytes, None)

    for what, kw in (("null", {"streams": None}), ("null", {"lens": None}), ("null", {"files": None}), ("null", {"file_len": None}),
                     ("null", {"ws_ptr": None}), ("positive", {"n": 0}), ("65535", {"h": 0}), ("65535", {"w": 65536}),
                     ("cap", {"cap": 0}), ("file_cap", {"file_cap": still - 1}), ("file_cap", {"animate": 1, "file_cap": movie - 1}),
                     ("ws holds", {"ws_bytes": ws - 1}), ("aligned", {"ws_ptr": p + 4}), ("aligned", {"lens": p + 2}),
                     ("aligned", {"file_len": p + 1}), ("delay", {"animate": 1, "file_cap": movie, "num": 0}),
                     ("delay", {"animate": 1, "file_cap": movie, "num": 65536}), ("delay", {"animate": 1, "file_cap": movie, "den": -1}),
                     ("delay", {"animate": 1, "file_cap": movie, "den": 65536}),
                     ("int32", {"animate": 1, "n": 3, "cap": 2 ** 30, "file_cap": 2 ** 33, "ws_bytes": 2 ** 30})):
        assert wrap(**kw) == -1, kw
        assert what in hip.last_error(), (kw, hip.last_error())

    crc_ws = lib.sp_crc32_ws_bytes(n, 50001)

    def crc(data=p, pitch=50001, lens=p, seed=None, n=n, out=p, ws_ptr=p, ws_bytes=crc_ws):
        return lib.sp_crc32_rows(data, pitch, lens, seed, n, out, ws_ptr, ws_bytes, None)

    for what, kw in (("null", {"data": None}), ("null", {"lens": None}), ("null", {"out": None}), ("null", {"ws_ptr": None}),
                     ("positive", {"n": 0}), ("pitch", {"pitch": 0}), ("pitch", {"pitch": 2 ** 31}), ("ws holds", {"ws_bytes": crc_ws - 1}),
                     ("aligned", {"lens": p + 1}), ("aligned", {"seed": p + 2}), ("aligned", {"out": p + 3}), ("aligned", {"ws_ptr": p + 2})):
        assert crc(**kw) == -1, kw
        assert what in hip.last_error(), (kw, hip.last_error())
