// svt-av1-1_amd/csrc/tq_tx_search_tu.h -- a search TU of the RD transform-type decision on the device (launch_tx_decision, tq_launch.h), in a
// header of its own so that md_full_kernels.h, which the host test compiles without the HIP runtime, can fill it.
#pragma once
#include <stdint.h>

namespace svthip {

// index[t] = the position of its TxType-t candidate inside the (tx_size, t) run of the launch order (0xffffffff: not a candidate),
// bases[tx_size * 16 + t] = where that run starts.
struct tx_search_tu_dev {
    uint64_t lambda;
    uint32_t index[16];
    uint32_t tx_size;
    uint32_t reserved;
};

}  // namespace svthip
