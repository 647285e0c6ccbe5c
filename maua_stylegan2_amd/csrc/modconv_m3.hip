// Instances of modconv_mfma_kernel for mode 3, Winograd F(4,3) along x.
#include "modconv_kernel.h"

#define MAUA_CONV_ROWS(X)                                                                          \
    MAUA_CONV_BOTH(X, 64, 128, 1, 3, 3)                                       /* F(4,3) */         \
    MAUA_CONV_BOTH(X, 32, 128, 1, 3, 3)
namespace {
const ConvInstance kConvInstances[] = {MAUA_CONV_ROWS(MAUA_CONV_ENTRY)};
}  // namespace
ConvTable maua_conv_table_m3() { return {kConvInstances, (int)(sizeof(kConvInstances) / sizeof(kConvInstances[0]))}; }
