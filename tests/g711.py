"""ITU-T G.711 written out for the tests: the expansion tables of all 256 codes
and the G.191 compression of all 65,536 samples, which the host twins
(tests/test_input_host.py, tests/test_output_host.py) are pinned to and the GPU
tests convert with.  Plain module."""
import numpy as np

import singlecarrier_amd as sc


def ulaw_table():
    """ITU-T G.711 mu-law, all 256 codes, written out here"""
    t = np.zeros(256, np.int64)
    for code in range(256):
        u = ~code & 0xFF
        m = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
        t[code] = 0x84 - m if u & 0x80 else m - 0x84
    return t


def alaw_table():
    """ITU-T G.711 A-law, all 256 codes, written out here"""
    t = np.zeros(256, np.int64)
    for code in range(256):
        a = code ^ 0x55
        m, s = (a & 15) << 4, (a >> 4) & 7
        v = m + 8 if s == 0 else m + 0x108 if s == 1 else (m + 0x108) << (s - 1)
        t[code] = v if a & 0x80 else -v
    return t


TABLES = {sc.IN_ALAW: alaw_table(), sc.IN_ULAW: ulaw_table()}


def expand(block, enc):
    """source elements -> int16, by this file's tables"""
    return block.astype(np.int16) if enc == sc.IN_S16 else TABLES[enc][block].astype(np.int16)


def _msb(v):
    return v.bit_length() - 1


def ulaw_compress(x):
    """ITU-T G.191 ulaw_compress on a 16-bit sample, written out here"""
    m = (~x >> 2) if x < 0 else (x >> 2)
    a = min(m + 33, 0x1FFF)
    s = _msb(a) - 4
    assert 1 <= s <= 8
    code = ((8 - s) << 4) | (15 - ((a >> s) & 15))
    return code | 0x80 if x >= 0 else code


def alaw_compress(x):
    """ITU-T G.191 alaw_compress on a 16-bit sample, written out here"""
    m = (~x >> 4) if x < 0 else (x >> 4)
    v = m
    if m >= 16:
        e = _msb(m) - 3
        v = (m >> (e - 1)) - 16 + (e << 4)
    if x >= 0:
        v |= 0x80
    return v ^ 0x55


ALL = np.arange(-32768, 32768, dtype=np.int64)
CODES = {sc.OUT_ALAW: np.array([alaw_compress(int(x)) for x in ALL], np.uint8),
         sc.OUT_ULAW: np.array([ulaw_compress(int(x)) for x in ALL], np.uint8)}


def compress(x, enc):
    """int16 samples -> elements of the encoding, by this file's formulas"""
    return x.astype(np.int16) if enc == sc.OUT_S16 else CODES[enc][x.astype(np.int64) + 32768]
