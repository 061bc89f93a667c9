"""Inputs of the tests of the conversion with the level meter in its pass and
of the squelched calls for every input format (tests/test_meter_host.py on the
CPU, tests/test_gpu_meter_fused.py on the GPU), written from
include/qpsk_input.h and include/qpsk_level.h alone.  Plain module."""
import functools

import numpy as np

import singlecarrier_amd as sc
from g711 import compress, expand
from level_cases import SINGLE_AT, oracle_case, restate_level, rows, silence_case

N = sc.FRAME_SIZE
TILE = 128   # samples of a time tile of the interleaved conversion
# the loudest and the quietest code of each encoding (A-law has no zero: +-8)
LOUD = {sc.IN_ALAW: (0xAA, 0x2A), sc.IN_ULAW: (0x80, 0x00)}
QUIET = {sc.IN_ALAW: 0xD5, sc.IN_ULAW: 0xFF}
LOUDEST = {sc.IN_ALAW: 32256, sc.IN_ULAW: 32124}


def tile_edges(f: int) -> list:
    """the samples of frame f on either side of each tile edge inside it"""
    first = -(f * N) % TILE or TILE
    at = []
    for e in range(first, N, TILE):
        at += [e - 1, e]
    return at


def block(enc: int, nch: int, nf: int, seed: int) -> np.ndarray:
    """[nch][nf][1880] elements of the encoding (uint8 codes or int16): random
    over every value, and by the row's number rows of the loudest code, of the
    quietest, of a single loud one at the ends of a row's first and last 16-byte
    words, and of a single loud one on either side of each tile edge"""
    rng = np.random.default_rng(seed)
    if enc == sc.IN_S16:
        x = rows(nch * nf, seed).reshape(nch, nf, N).copy()   # rails and special rows included
        quiet, loud = 0, (32767, -32768)
    else:
        x = rng.integers(0, 256, (nch, nf, N)).astype(np.uint8)
        quiet, loud = QUIET[enc], LOUD[enc]
    for r in range(nch * nf):
        c, f = divmod(r, nf)
        kind = r % 7
        if kind == 1 and enc != sc.IN_S16:
            x[c, f] = loud[r % 2]
        elif kind == 2 and enc != sc.IN_S16:
            x[c, f] = quiet
        elif kind in (3, 4):
            x[c, f] = quiet
            at = SINGLE_AT if kind == 3 else tile_edges(f)
            x[c, f, at[r % len(at)]] = loud[r % 2]
            if r % 3 == 0:
                x[c, f, list(at)] = loud[0]
    return x


def source(x: np.ndarray, layout: int, ld: int, seed: int = 0) -> np.ndarray:
    """the block as a flat source: planar [nch][T], or interleaved [T][ld] with
    loud elements in the columns past nch (they are not the block's)"""
    nch, nf, _ = x.shape
    T = nf * N
    if layout == sc.IN_PLANAR:
        return np.ascontiguousarray(x.reshape(nch * T))
    rng = np.random.default_rng(seed + 1)
    wide = rng.integers(0, 256, (T, ld)).astype(x.dtype) if x.dtype == np.uint8 else \
        rng.choice(np.array([32767, -32768], np.int16), (T, ld))
    wide[:, :nch] = x.reshape(nch, T).T
    return np.ascontiguousarray(wide.reshape(-1)[:(T - 1) * ld + nch])


def decoded(x: np.ndarray, enc: int) -> np.ndarray:
    """int16 of a block of elements, by the tests' own tables (g711.py)"""
    return x.astype(np.int16) if enc == sc.IN_S16 else expand(x, enc)


@functools.lru_cache(maxsize=None)
def format_case(enc: int, mode: int = 0):
    """level_cases.oracle_case compressed to the encoding: (elements
    [8][8][1880], the decoded samples, the oracle's dense outputs for them,
    their levels by numpy); read-only, made once"""
    import rxcheck
    x, d, level = oracle_case(mode)
    if enc == sc.IN_S16:
        return x, x, d, level
    codes = compress(x, enc).astype(np.uint8)
    y = np.ascontiguousarray(expand(codes, enc).astype(np.int16))
    d = rxcheck.expected(y, mode)
    level = restate_level(y)
    for a in (codes, y, level):
        a.setflags(write=False)
    return codes, y, d, level


@functools.lru_cache(maxsize=None)
def silence_format_case(enc: int):
    """level_cases.silence_case as elements of the encoding: the quietest code
    in every sample (mu-law and int16: zero; A-law: 8, it has no zero)"""
    import rxcheck
    x, d = silence_case(0)
    if enc == sc.IN_S16:
        return x, x, d
    codes = np.full(x.shape, QUIET[enc], np.uint8)
    y = np.ascontiguousarray(expand(codes, enc).astype(np.int16))
    return codes, y, (d if not y.any() else rxcheck.expected(y, 0))


def as_layout(x: np.ndarray, layout: int) -> np.ndarray:
    """[nch][nf][1880] elements as the array the Python calls take: planar
    [nch][T] or interleaved [T][nch]"""
    nch, nf, _ = x.shape
    p = x.reshape(nch, nf * N)
    return np.ascontiguousarray(p.T if layout == sc.IN_INTERLEAVED else p)
