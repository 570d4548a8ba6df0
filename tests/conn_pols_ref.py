"""The checker of the connection polynomials: a plain transcription of the two loops the compressor and final setups run
(src/compressor/compressor12_setup.js:470-500 and its siblings) over Python integers -- the identity columns S[j][i] = w^i ks'[j], then the
SEQUENTIAL swaps `connect(S[first.col], first.row, S[j], i)` (polutils.js:166) with the table of first sightings.  It does not know the closed
form the library uses, so the tests check that form.  Both fields: values are integers mod q; Fr values turn into Montgomery words only at
the comparison (fr_mont_words).  Nothing here touches the library."""
import random

import numpy as np

P = 0xFFFFFFFF00000001
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
GL_W32 = 7277203076849721926          # F.w[32] of f3g.js:30-35; F.w[b] = GL_W32^(2^(32 - b))
GL_K = 12275445934081160404           # F.k, f3g.js:26
FR_W28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904      # a 2^28-th root of unity of BN254 Fr
FR_K = 5


def root(q, n_bits):
    return pow(GL_W32, 1 << (32 - n_bits), P) if q == P else pow(FR_W28, 1 << (28 - n_bits), R)


def get_ks(q, n):
    """ks[i] = k^(i + 1), the shape of pilcom's getKs"""
    k = GL_K if q == P else FR_K
    return [pow(k, i + 1, q) for i in range(n)]


def conn_pols(s_map, n_rows, n_cols, N, w, ks, q):
    """s_map[i * n_cols + j] for i < n_rows; -> S as S[j][i], integers mod q"""
    S = [[0] * N for _ in range(n_cols)]
    x = 1
    for i in range(N):
        S[0][i] = x
        for j in range(1, n_cols):
            S[j][i] = x * ks[j - 1] % q
        x = x * w % q
    last_signal = {}
    for i in range(n_rows):
        for j in range(n_cols):
            s = s_map[i * n_cols + j]
            if s:
                if s in last_signal:
                    col, row = last_signal[s]
                    S[col][row], S[j][i] = S[j][i], S[col][row]          # connect: a swap
                else:
                    last_signal[s] = (j, i)
    return S


def rows(S):
    """S[j][i] -> [i][j], the library's row-major order"""
    return [list(r) for r in zip(*S)] if S else []


def gl_words(S):
    return np.array(rows(S), np.uint64)


def fr_words(vals):
    """integers below 2^256 -> (n, 4) uint64, as they are"""
    a = np.zeros((len(vals), 4), np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            a[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return a


def to_mont(v):
    return v % R * MONT % R


def fr_mont_words(S):
    """S[j][i] -> (N, nCols, 4) Montgomery words"""
    r = rows(S)
    return fr_words([to_mont(v) for row in r for v in row]).reshape(len(r), len(S), 4)


def words(S, q):
    return gl_words(S) if q == P else fr_mont_words(S)


def consts(w, ks, q):
    """(w, ks) as the library takes them: uint64 words, Montgomery for Fr"""
    if q == P:
        return np.array([w], np.uint64), np.array(ks, np.uint64)
    return fr_words([to_mont(w)]), fr_words([to_mont(k) for k in ks])


def rng(seed):
    return random.Random(seed)
