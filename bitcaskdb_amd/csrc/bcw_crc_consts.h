// bcw_crc_consts.h -- the shapes of the CRC-32C constant tables: what the kernels index (through bcw_internal.h) and
// what the host builds (bcw_crc_tables.h). Plain C++, no HIP.
#pragma once

namespace bcw {

// shift operators A_{8 * 2^k} for k < kPow2Ops: any shift below 2^16 bytes (a fragment's u16 length)
constexpr int kPow2Ops = 16;

// enc_ops layout (operators of 128 words): [n] A_{8*16*n}, [16 + n] A_{8*256*n} (n < 16), [32 + n]
// A_{8*4096*n} (n < 8), [40 + t] A_{8t}^-1 (t < 16), [56 + k] A_{8*2^k} (k < 32), [88 + k] A_{8*2^k}^-1 (k < 15)
constexpr int kOpInv = 40, kOpPow2 = 56, kOpPow2Inv = 88;
constexpr int kEncOpsWords = 103 * 128;

// k_crc stream verify (bcw_decode.hip, stream_verify): absolute 1 KiB chunks, 16 B per lane (one fully contiguous
// load per chunk). LDS image (dwords): the lane operators G_l = A_{8*16*(63-l)} transposed to [8][16][64 lanes]
// (first: byte offsets i * 4096 + v * 256 + 4 l, each table base a ds_read immediate); slice-by-4 rows of 256 B
// {T3, T2, T1, T0} x 8 copies then the shifted tables T'_k (a byte followed by k + 1008 zero bytes) x 8 copies; the
// split operators A_{8*(4*(4-k) + 1008)} (k = 0..3) as byte tables [k][byte t][256]; and the per-lane byte-select
// tables of the fragment-end masks (16 B entries, one per lane offset): GE (bytes >= n), JSEL (the check word's bytes
// at piece offset m - 3), GAP (check word at piece offset g - 6, then 3 zero bytes).
constexpr int kSPiece = 16;
constexpr int kSChunk = 64 * kSPiece;
constexpr int kSPW = kSPiece / 4;  // words per lane
constexpr int kS2Slice = 256 * 64, kS2Lop = 8 * 16 * 64, kS2Kop = kSPW * 4 * 256;
constexpr int kS2LopOff = 0, kS2SliceOff = kS2Lop, kS2KopOff = kS2Lop + kS2Slice;
constexpr int kS2GeN = 17, kS2JselN = 20, kS2GapN = 23;  // entries (4 dwords each)
constexpr int kS2Ge = kS2Slice + kS2Lop + kS2Kop, kS2Jsel = kS2Ge + 4 * kS2GeN, kS2Gap = kS2Jsel + 4 * kS2JselN;
constexpr int kS2Image = kS2Gap + 4 * kS2GapN + 4;  // (+ pad to 16 B)

}  // namespace bcw
