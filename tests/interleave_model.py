"""Numpy model of the interleaver and the scrambler of include/ofdm_mi355x.h
("interleaver and scrambler"): the definition the GPU kernels are tested
against; test_interleave_model.py pins it to the 802.11a facts.

perm(n, c, s)[q] is the position j that block position q moves to. Arrays are
interleaved along their last axis, block by block."""
import functools

import numpy as np

MAX_BLOCK = 32768


def valid(n, c, s):
    return (8 <= n <= MAX_BLOCK and n % 8 == 0 and c >= 1 and n % c == 0 and s >= 1 and (n // c) % s == 0)


@functools.lru_cache(maxsize=None)
def perm(n, c, s):
    assert valid(n, c, s), (n, c, s)
    q = np.arange(n, dtype=np.int64)
    i = (n // c) * (q % c) + q // c
    j = s * (i // s) + (i + n - (c * i) // n) % s
    j.setflags(write=False)
    return j


@functools.lru_cache(maxsize=None)
def inverse_perm(n, c, s):
    """The closed form of the header: inverse_perm[j] = q."""
    assert valid(n, c, s), (n, c, s)
    j = np.arange(n, dtype=np.int64)
    i = s * (j // s) + (j + (c * j) // n) % s
    q = c * i - (n - 1) * ((c * i) // n)
    q.setflags(write=False)
    return q


def _blocks(x, n):
    x = np.asarray(x)
    assert x.shape[-1] % n == 0
    return x.reshape(x.shape[:-1] + (x.shape[-1] // n, n))


def interleave(x, n, c, s):
    """out[j(q)] = in[q] in every block of n along the last axis."""
    b = _blocks(x, n)
    out = np.empty_like(b)
    out[..., perm(n, c, s)] = b
    return out.reshape(np.asarray(x).shape)


def deinterleave(x, n, c, s):
    """out[q] = in[j(q)]."""
    b = _blocks(x, n)
    return b[..., perm(n, c, s)].reshape(np.asarray(x).shape)


def scramble_sequence(seed, nbits):
    """s_t = s_{t-4} ^ s_{t-7}, s_{-m} = bit m-1 of the seed (1..127)."""
    assert 1 <= seed <= 127
    hist = [(seed >> (m - 1)) & 1 for m in range(1, 8)]  # hist[m-1] = s_{t-m}
    out = np.zeros(nbits, np.uint8)
    for t in range(nbits):
        b = hist[3] ^ hist[6]
        out[t] = b
        hist = [b] + hist[:6]
    return out


def reduce_seed(v):
    """A per-codeword seed byte as the device reads it."""
    return (int(v) - 1) % 127 + 1


def scramble(bits, seeds):
    """(ncw, nbits) bits XOR the sequence of seeds[cw] (a scalar: every row)."""
    bits = np.atleast_2d(np.asarray(bits, np.uint8))
    seeds = np.broadcast_to(np.asarray(seeds), (bits.shape[0],))
    seq = np.stack([scramble_sequence(reduce_seed(v), bits.shape[1]) for v in seeds])
    return bits ^ seq
