"""Numpy model of the channel code of include/ofdm_mi355x.h ("channel code"):
the K=7 133/171 convolutional encoder with its 2/3 and 3/4 puncturings and a
soft-input Viterbi decoder, vectorised over codewords and states. The model
is the definition the GPU kernels are tested against; test_fec_model.py pins
it to the textbook facts.

Bits travel as uint8 arrays of 0/1, shape (ncw, nbits); pack() / unpack() go
to the MSB-first bytes of the C ABI."""
import numpy as np

R12, R23, R34 = 0, 1, 2
RATES = (R12, R23, R34)
KEEP = {R12: (1,), R23: (1, 1, 1, 0), R34: (1, 1, 1, 0, 0, 1)}
GEN_A, GEN_B = 0o133, 0o171
TAIL = 6
UNREACHABLE = -(1 << 40)


def _parity(x):
    x = np.asarray(x)
    p = np.zeros_like(x)
    for b in range(7):
        p ^= (x >> b) & 1
    return p


def steps(info_bits):
    return info_bits + TAIL


def kept_positions(info_bits, rate):
    """Mother-stream indices (ascending) of the transmitted bits."""
    keep = KEEP[rate]
    i = np.arange(2 * steps(info_bits))
    return i[np.array(keep)[i % len(keep)] == 1]


def coded_bits(info_bits, rate):
    return len(kept_positions(info_bits, rate))


def max_info_bits(capacity_bits, rate):
    """Largest info_bits whose codeword fits, or None."""
    best = None
    n = 1
    while coded_bits(n, rate) <= capacity_bits:
        best = n
        n += 1
    return best


def encode_mother(info):
    """(ncw, info_bits) bits -> (ncw, 2T) mother stream A0 B0 A1 B1 ..."""
    info = np.atleast_2d(np.asarray(info, np.uint8))
    ncw, nb = info.shape
    u = np.concatenate([info, np.zeros((ncw, TAIL), np.uint8)], axis=1).astype(np.int64)
    state = np.zeros(ncw, np.int64)
    m = np.zeros((ncw, 2 * steps(nb)), np.uint8)
    for t in range(steps(nb)):
        reg = (u[:, t] << 6) | state
        m[:, 2 * t] = _parity(reg & GEN_A)
        m[:, 2 * t + 1] = _parity(reg & GEN_B)
        state = reg >> 1
    return m


def encode(info, rate):
    """(ncw, info_bits) bits -> (ncw, coded_bits) transmitted bits."""
    info = np.atleast_2d(np.asarray(info, np.uint8))
    return encode_mother(info)[:, kept_positions(info.shape[1], rate)]


def depuncture(llr, info_bits, rate):
    """(ncw, coded_bits) LLRs -> (ncw, T, 2) with 0 at the punctured positions."""
    llr = np.atleast_2d(llr)
    full = np.zeros((llr.shape[0], 2 * steps(info_bits)), llr.dtype)
    full[:, kept_positions(info_bits, rate)] = llr[:, :coded_bits(info_bits, rate)]
    return full.reshape(llr.shape[0], -1, 2)


def _branches():
    """For new state s' and j: predecessor p_j and the branch's (A, B)."""
    sp = np.arange(64)
    out = []
    for j in (0, 1):
        p = ((2 * sp) & 63) | j
        reg = ((sp >> 5) << 6) | p
        out.append((p, _parity(reg & GEN_A), _parity(reg & GEN_B)))
    return out


def viterbi(llr, info_bits, rate):
    """Soft-input Viterbi. llr: (ncw, >= coded_bits), integer (int64 metrics)
    or real (float64 metrics); L > 0 means bit 0. Returns (info bits
    (ncw, info_bits) uint8, the best path's metric (ncw,))."""
    llr = np.atleast_2d(np.asarray(llr))
    mt = np.int64 if np.issubdtype(llr.dtype, np.integer) else np.float64
    L = depuncture(llr.astype(mt), info_bits, rate)
    ncw, T, _ = L.shape
    pm = np.full((ncw, 64), UNREACHABLE, mt)
    pm[:, 0] = 0
    (p0, a0, b0), (p1, a1, b1) = _branches()
    sa0, sb0, sa1, sb1 = (1 - 2 * a0).astype(mt), (1 - 2 * b0).astype(mt), (1 - 2 * a1).astype(mt), (1 - 2 * b1).astype(mt)
    dec = np.zeros((ncw, T, 64), np.uint8)
    for t in range(T):
        la, lb = L[:, t, 0:1], L[:, t, 1:2]
        c0 = pm[:, p0] + (sa0 * la + sb0 * lb)
        c1 = pm[:, p1] + (sa1 * la + sb1 * lb)
        d = c1 > c0  # a tie keeps j = 0
        dec[:, t] = d
        pm = np.where(d, c1, c0)
    best = pm[:, 0].copy()
    s = np.zeros(ncw, np.int64)
    rows = np.arange(ncw)
    bits = np.zeros((ncw, T), np.uint8)
    for t in range(T - 1, -1, -1):
        bits[:, t] = s >> 5
        s = ((s << 1) & 63) | dec[rows, t, s]
    return bits[:, :info_bits], best


def path_metric(info, llr, rate):
    """Metric sum (1 - 2 c_n) L_n of the codeword of `info` (float64 or int64)."""
    info = np.atleast_2d(np.asarray(info, np.uint8))
    llr = np.atleast_2d(np.asarray(llr))
    mt = np.int64 if np.issubdtype(llr.dtype, np.integer) else np.float64
    c = encode(info, rate).astype(mt)
    return ((1 - 2 * c) * llr[:, :c.shape[1]].astype(mt)).sum(axis=1)


def pack(bits):
    """(ncw, nbits) bits -> (ncw, ceil(nbits/8)) bytes, MSB first, zero-padded."""
    return np.packbits(np.atleast_2d(np.asarray(bits, np.uint8)), axis=1)


def unpack(data, nbits):
    """(ncw, >= ceil(nbits/8)) bytes -> (ncw, nbits) bits."""
    return np.unpackbits(np.atleast_2d(np.asarray(data, np.uint8)), axis=1)[:, :nbits]
