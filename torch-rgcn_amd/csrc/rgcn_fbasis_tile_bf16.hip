// bf16 storage for the tile kernels of rgcn_fbasis_tile.hip: the same kernels instantiated for a bf16 table, gradient and
// upstream gradient, in a translation unit of their own -- rgcn_fbasis_tile_fwd_bf16, rgcn_gather_rows_sum4_bf16, rgcn_fbasis_tile_bwd_bf16
#define RGCN_FBT_BF16 1
#include "rgcn_fbasis_tile.hip"
