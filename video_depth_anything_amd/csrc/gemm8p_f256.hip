// 8-phase two-group schedule of the 256 x 256 tile, conv A on the tap grid of a folded ConvTranspose (VDA_EPI_CONVT_FOLD_F16).
#include "gemm8p_kernel.h"

int vda_gemm8p_conv_fold_bn256(const vda_gemm_args& a, hipStream_t s) { return vda_gemm8p::launch_conv_fold<256>(a, s); }
