// ofdm_interleave.hpp — index arithmetic of the block interleaver of
// include/ofdm_mi355x.h ("interleaver and scrambler"), shared by the kernels
// of ofdm_interleave.hip and by the launch code that sizes their LDS image.
// Plain C++: host code can include it without the HIP runtime.
#pragma once

#if defined(__HIPCC__)
#define OFDM_IL_HD __host__ __device__
#else
#define OFDM_IL_HD
#endif

namespace ofdm {

// Walks the positions of one block in ascending order and gives, for each,
// the position its value is gathered from. A block is c columns of
// rows = n/c positions, and s divides rows, so floor(c*i/n) of the header's
// formulas is the column of i and every modulo below is a counter:
//   DIR 0 (forward, out[j] = in[q]):  j = rows*col + jr,
//       i = j - jr%s + (jr%s + col%s) % s,  q = c*(i - rows*col) + col
//   DIR 1 (inverse, out[q] = in[j]):  q = c*row + col,  i = rows*col + row,
//       j = i - row%s + (row%s - col%s) mod s
// a is the fast counter (jr, or col), b the slow one (col, or row); am, bm are
// a % s and b % s. Past the block's last position the walk is at position 0
// of the next block (every counter is 0 there).
template <int DIR>
struct IlWalk {
    int c, rows, s, a, b, am, bm;

    OFDM_IL_HD IlWalk(int c_, int rows_, int s_, int p) : c(c_), rows(rows_), s(s_)
    {
        const int lim = DIR == 0 ? rows : c;
        b = p / lim;
        a = p - b * lim;
        am = a % s;
        bm = b % s;
    }
    OFDM_IL_HD int src() const
    {
        if (DIR == 0) {
            int t = am + bm;
            if (t >= s) t -= s;
            return c * (a - am + t) + b;
        }
        int t = bm - am;
        if (t < 0) t += s;
        return rows * a + b - bm + t;
    }
    // true when the step left the block
    OFDM_IL_HD bool next()
    {
        const int lim = DIR == 0 ? rows : c, lim2 = DIR == 0 ? c : rows;
        if (++am == s) am = 0;
        if (++a < lim) return false;
        a = 0;
        am = 0;
        if (++bm == s) bm = 0;
        if (++b < lim2) return false;
        b = 0;
        bm = 0;
        return true;
    }
};

// The staged image's padding: byte x of a tile sits at x + (x >> shift) * pad
// (pad a multiple of 4 and shift >= 2, so a 4-byte word never straddles a pad;
// shift = 31: no padding).
struct IlPad {
    unsigned shift, pad;
    OFDM_IL_HD unsigned at(unsigned x) const { return x + (x >> shift) * pad; }
};

}  // namespace ofdm
