// Instances of modconv_mfma_kernel for mode 1, transposed (polyphase).
#include "modconv_kernel.h"

#define MAUA_CONV_ROWS(X)                                                                          \
    MAUA_CONV_BOTH(X, 32, 128, 1, 1, 1) MAUA_CONV_BOTH(X, 32, 128, 1, 1, 2)   /* transposed */     \
    MAUA_CONV_BOTH(X, 64, 64, 2, 1, 1) X(64, 64, 2, 1, true, 2)
namespace {
const ConvInstance kConvInstances[] = {MAUA_CONV_ROWS(MAUA_CONV_ENTRY)};
}  // namespace
ConvTable maua_conv_table_m1() { return {kConvInstances, (int)(sizeof(kConvInstances) / sizeof(kConvInstances[0]))}; }
