// svt-av1-1_amd/csrc/me_fullpel_img2.h -- the two-image entry of the 85-PU full-pel search (me_fullpel.hip): its LDS plan and
// launch_fullpel's choice between it and fullpel85_kernel.
#pragma once
#include "me_fullpel_common.h"

// Launches whose search areas are at most 64x64 keep TWO images of the reference window in LDS, the second one read 4 bytes later, so
// that the odd dword pairs of a window row (W1,W2), (W3,W4), (W5,W6) are naturally aligned wide reads like the even ones and no
// register moves are needed in front of v_qsad_pk_u16_u8 (a 64-bit VGPR operand starts at an even register).
// Pitch 144 B = 36 dwords: 4 * 36 = 16, 8 * 36 = 32, 12 * 36 = 48 (mod 64), so window rows r, r+4, r+8, r+12 start on the four quarters
// of the 64 banks -- the lane -> row map of the search loop puts exactly such rows into one 16-lane ds_read_b128 group
// (tools/fullpel_lane_map_check.py).  144 B also hold the widest lane footprint of a 64-wide area (bytes 96 .. 127 of image 0,
// 100 .. 131 of the window through image 1).  Both images always take 127 rows: 16 448 + 2 * 127 * 144 = 53 024 B per workgroup, three
// workgroups per CU (160 KiB / 3 = 54 613 B) and below the 64 KiB from which a launch needs a function attribute.
// SVTHIP_FULLPEL_LDS_PITCH stays what it is: fullpel85_kernel and fullpel209_kernel share it.
#define SVTHIP_FULLPEL_IMG2_PITCH 144
#define SVTHIP_FULLPEL_IMG2_ROWS 127
#define SVTHIP_FULLPEL_IMG2_MAX_AREA 64

namespace svthip {

// fullpel85_img2_kernel: same arguments and results as fullpel85_kernel; every superblock of the launch must have a search area of at
// most 64x64
inline bool fullpel_img2_fits(uint32_t max_sw, uint32_t max_sh)
{
    return max_sw <= SVTHIP_FULLPEL_IMG2_MAX_AREA && max_sh <= SVTHIP_FULLPEL_IMG2_MAX_AREA;
}
inline size_t fullpel_img2_lds_bytes()
{
    return SVTHIP_FULLPEL_LDS_FIXED + 2 * (size_t)SVTHIP_FULLPEL_IMG2_ROWS * SVTHIP_FULLPEL_IMG2_PITCH;
}

}  // namespace svthip
