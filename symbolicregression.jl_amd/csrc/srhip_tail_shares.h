// The persistent launch's last round as equal shares ("Block size and tail").
//
// The nmain row blocks of a persistent launch on wgs workgroups: the first nfull = (nmain / wgs) * wgs
// are claimed whole.  The Lb = nmain - nfull leftover blocks are cut into S units each -- unit u of a
// block is its order slots with slot % S == u; the order is by descending cost, so the units of a block
// cost about the same -- and the N = Lb * S units, block-major, into nshares contiguous ranges of
// near-equal length: share w is units [floor(w N / nshares), floor((w + 1) N / nshares)).  One share is
// one claimed item.  With nshares >= Lb a share is at most S units long, so it lies in at most two
// blocks: at most two parts (block, u0, u1), each one staged block and one pass over the trees of its
// units.  Whole blocks of S-unit slices claimed one by one end the round after ceil(Lb S / wgs) / S
// block times -- for C2 (Lb = 229, wgs = 256) 1.0 at S = 8 and 15/16 at S = 16, no better than whole
// blocks -- while shares end it after ceil(Lb S / wgs) / S = 58/64 at S = 64, 115/128 at S = 128, with
// ONE staging per part, not one per unit.
//
// Included by the host (plan, tests' C entry point) and by the interpreter kernel (item decode): plain
// 32-bit arithmetic, the host keeps Lb * S * nshares below 2^31.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SRHIP_SHARES_HD __host__ __device__
#else
#define SRHIP_SHARES_HD
#endif

namespace srhip {

struct TailPart {
  int32_t block;   // leftover block, 0 .. Lb - 1
  int32_t u0, u1;  // its units [u0, u1), 0 <= u0 < u1 <= S
};

// The parts of share w (0 <= w < nshares, nshares >= Lb >= 1): returns their number, 0 (an empty share:
// fewer units than shares), 1 or 2.
SRHIP_SHARES_HD inline int tail_share_parts(int32_t Lb, int32_t S, int32_t nshares, int32_t w, TailPart out[2]) {
  const int32_t N = Lb * S;
  const int32_t a = (int32_t)((uint32_t)w * (uint32_t)N / (uint32_t)nshares);
  const int32_t b = (int32_t)((uint32_t)(w + 1) * (uint32_t)N / (uint32_t)nshares);
  if (b <= a) return 0;
  const int32_t blk = a / S;
  const int32_t u0 = a - blk * S;
  const int32_t end = (blk + 1) * S;  // first unit of the next block
  out[0].block = blk;
  out[0].u0 = u0;
  out[0].u1 = (b < end ? b : end) - blk * S;
  if (b <= end) return 1;
  out[1].block = blk + 1;
  out[1].u0 = 0;
  out[1].u1 = b - end;
  return 2;
}

// Order slots below n whose unit (slot % S) lies in [u0, u0 + w): tree index ti of such a group, in
// ascending slot order, is slot (ti / w) * S + u0 + ti % w.  (w = 1: the slots u0, u0 + S, ...)
SRHIP_SHARES_HD inline int32_t tail_units_count(int32_t n, int32_t S, int32_t u0, int32_t w) {
  const int32_t rem = n % S - u0;
  return n / S * w + (rem < 0 ? 0 : (rem < w ? rem : w));
}

}  // namespace srhip
