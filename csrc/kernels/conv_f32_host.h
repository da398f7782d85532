// Host-side helpers that more than one fp32 conv unit (conv_f32_*.hip) calls; defined in conv_f32_pool.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "kernels.h"

namespace ringdp::kern {
constexpr int kSlabGroup = 32;  // slices per stage-1 group of the fixed-order slab sums (conv_f32_wgrad.hip)
constexpr int kP2Tile = 16;     // planes per workgroup tile of pool2s1_bwd_tile_kernel
int f32_num_cus();
int grid_1d(int64_t n);
int grid_elems(int64_t n);
int64_t batch_chunk(int64_t B, std::initializer_list<int64_t> per_image);
// The ConvNet's conv2 (32 -> 64 channels, 3x3 valid, 13x13 -> 11x11) and conv3 (64 -> 128, 10x10 -> 8x8), the
// geometries with dedicated kernels; each user adds its own batch threshold and 32-bit bound
bool is_convnet_conv2(const ConvF32Geom& g);
bool is_convnet_conv3(const ConvF32Geom& g);
// pool2s1_bwd_tile_kernel over ntiles tiles of kP2Tile planes; slices > 1: da is that many split-K planes of
// `plane` floats each, summed in order as a tile is staged
void pool2s1_bwd_tile(const float* da, const unsigned char* code, float* dz, int ntiles, int PH, int PW, int slices,
                      int64_t plane, hipStream_t s);
}  // namespace ringdp::kern
