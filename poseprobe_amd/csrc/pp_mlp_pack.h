// Layout of the object-branch MLP weight pack (pp_mlp_pack, include/poseprobe_hip.h): everything the prologues of the five
// split-precision data-path kernels (pp_mlp_split.hip) derive from the parameters, computed once by k_mlp_pack and read back with
// 16-byte loads.  Offsets in floats.  A hidden layer's image holds, for thread `tid` of a 256-thread work-group and operand
// group ks, the lane's hi registers at 16-byte slot (2 ks) * 256 + tid and its lo registers at slot (2 ks + 1) * 256 + tid.
#pragma once

#define PK_IMG 16384                              // one 128 x 128 layer as hi | lo fp16: as many bytes as its fp32 weights
#define PK_SCAL 0                                 // 64 scalar slots (exponents are stored as integer bits)
#define PK_WARP 64                                // warp net images: W1 W2 W3 (rows, forward) | W3 W2 W1 (columns, data gradient)
#define PK_RGB (PK_WARP + 6 * PK_IMG)             // rgbnet images: W0 (rows, 64 wide: half an image) W1 W2 | W2 W1 (columns) W0^T
#define PK_RGB_W1 (PK_RGB + PK_IMG / 2)
#define PK_FLOATS (PK_RGB_W1 + 5 * PK_IMG)

enum {  // scalar slots of the warp net
  PKW_EW1 = 0, PKW_L1_1, PKW_EW2, PKW_L1_2, PKW_EW3, PKW_L1_3, PKW_B1MX, PKW_B2MX, PKW_W0L1, PKW_W0MX, PKW_B0MX, PKW_EW0,
  PKW_EW3C, PKW_L1_3C, PKW_EW2C, PKW_L1_2C, PKW_EW1C, PKW_L1_1C,
  // ... and of rgbnet
  PKR_EW0 = 32, PKR_L1_0, PKR_EW1, PKR_L1_1, PKR_EW2, PKR_L1_2, PKR_B0MX, PKR_B1MX,
  PKR_EW2C, PKR_L1_2C, PKR_EW1C, PKR_L1_1C, PKR_EW0T, PKR_W3L1, PKR_EW3
};
#define PK_TASKS_WARP 7                           // work-groups of k_mlp_pack: one per image + one for the thin layers' scalars
#define PK_TASKS 14
