// tcgnn_internal.h - declarations shared by the host and device halves of libtcgnn_hip.so.
#ifndef TCGNN_INTERNAL_H
#define TCGNN_INTERNAL_H

#include <cstdarg>
#include <cstdint>

namespace tcgnn {

// Records a thread-local message for tcgnn_last_error() and returns `status`.
int fail(int status, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Geometry of the packed tile stream ("wide blocks": four 16x8 TC blocks side by side).
constexpr int kWinRows = 16;   // BLK_H
constexpr int kTcCols = 8;     // BLK_W
constexpr int kWbCols = 32;    // condensed columns per MFMA operand tile (K of 16x16x32)
constexpr int kMaxChunkDims = 128; // feature columns handled by one workgroup pass

// Launchers of the CSR transpose's hand-written kernels (tcgnn_transpose.inc, compiled into tcgnn_device.hip; the rocPRIM sort and the
// entry points are in tcgnn_transpose.hip).  Stream-ordered; each returns the hipError_t of its launch as an int.
int transpose_row_ids(const int32_t* rowptr, int32_t N, int64_t E, int32_t* rowid, void* stream);
int transpose_row_pointers(const uint32_t* sorted_keys, int64_t E, int32_t N, int32_t* rowptr_t, void* stream);
int transpose_gather_rows(const int32_t* perm, const int32_t* rowid, int64_t E, int32_t* col_t, void* stream);
int transpose_check(const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t, const int32_t* col_t, int32_t N, int64_t E,
                    uint32_t* res, void* stream);
int permute_edge_values(const float* val, const int32_t* perm, int64_t E, float* out, void* stream);

// Launchers of the neighbour sampler's kernels (tcgnn_sample.inc, compiled into tcgnn_device.hip; the entry points are in
// tcgnn_sample.hip).  Stream-ordered; each returns the hipError_t of its launch as an int.
int64_t sample_scan_blocks(int32_t N);   // words of scratch sample_count needs
int sample_count(const int32_t* rowptr, const uint8_t* mask, int32_t N, int64_t E, int32_t fanout, uint32_t* sums, uint32_t* res, int32_t* rowptr_s,
                 void* stream);
int sample_select(const int32_t* rowptr, const int32_t* col, const uint8_t* mask, const int32_t* rowptr_s, int32_t N, int64_t E, int32_t fanout,
                  uint64_t seed, int32_t* col_s, int32_t* eid, void* stream);
// the same over a list of R row ids (tcgnn_sample_rows*): the scan runs over the list, the select launches one workgroup per four slots
int64_t sample_rows_scan_blocks(int32_t R);   // words of scratch sample_rows_count needs
int sample_rows_count(const int32_t* rowptr, const int32_t* rows, int32_t R, int32_t N, int64_t E, int32_t fanout, uint32_t* sums, uint32_t* res,
                      int32_t* rowptr_s, void* stream);
int sample_rows_select(const int32_t* rowptr, const int32_t* col, const int32_t* rows, const int32_t* rowptr_s, int32_t R, int32_t N, int64_t E,
                       int32_t fanout, uint64_t seed, int32_t* col_s, int32_t* eid, void* stream);

} // namespace tcgnn
#endif
