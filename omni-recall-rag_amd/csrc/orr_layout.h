// orr_layout.h -- the byte layout of a text pool the scan kernels read (contents before the seal, the vocabulary after it):
// every row starts 16-byte aligned and is followed by 1..16 space bytes, and the pool is over-allocated by kScanPoolSlack
// bytes.  No HIP here: the host-side builders (orr_token_index.cpp, orr_insert_plan.h) lay pools out by the same rule.
#pragma once

#include <cstddef>
#include <cstdint>

namespace orr {

constexpr size_t kScanPoolSlack = 2048;
constexpr uint64_t kRowAlign = 16;
inline uint64_t padded_row_bytes(uint64_t len) { return (len / kRowAlign + 1) * kRowAlign; }

}  // namespace orr
