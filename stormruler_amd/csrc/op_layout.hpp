// Sizes of the operator's records: what the host packer (op_pack.hip) writes and the apply kernels (spmv_device.hpp and
// the units behind it) read.  Constants only; the layouts themselves: the header of spmv.hip.
#pragma once

#include "common.hpp"

namespace storm {

constexpr int kExtBytes = kWave * 8;      // 512
constexpr int kSlotBytes = kWave * 12;    // 768: one ELL slot of a slice (64 cols + 64 vals)
constexpr int kExt32Bytes = kWave * 4;    // 256: the fp32-weight companion record (sell_device.hpp Rec32, op_reduced.hip)
constexpr int kSlot32Bytes = kWave * 8;   // 512: one of its slots (64 cols + 64 f32 weights, interleaved)
constexpr int kDictSize = 256;
constexpr int kPairRecBytes = 2 * kWave * 8 + kWave * 8;  // format 3: 64 x (u64, u64) weights + 64 x u64 offsets per 128 rows
constexpr int kColSlotBytes = kWave * 4;  // 256: one slot of a value-dictionary record (columns only)
constexpr int kCanonRecBytes = 2 * kWave * 8;  // format 4: 64 x (u64, u64) weights per 128 rows

}  // namespace storm
