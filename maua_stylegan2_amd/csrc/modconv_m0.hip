// Instances of modconv_mfma_kernel for mode 0, direct 3x3.
#include "modconv_kernel.h"

#define MAUA_CONV_ROWS(X)                                                                          \
    MAUA_CONV_BOTH(X, 128, 128, 2, 0, 1) MAUA_CONV_BOTH(X, 128, 128, 2, 0, 2) /* direct 3x3 */     \
    MAUA_CONV_BOTH(X, 64, 256, 1, 0, 2)                                                            \
    MAUA_CONV_BOTH(X, 32, 256, 1, 0, 2)
// The tile configs only the A/B bits of an experiments build select (g_conv_cfg), with every MULTI x MAXP their patch limit allows.
#define MAUA_CONV_ROWS_EXPERIMENTS(X)                                                                          \
    MAUA_CONV_BOTH(X, 32, 512, 1, 0, 1) MAUA_CONV_BOTH(X, 32, 512, 1, 0, 2) MAUA_CONV_BOTH(X, 32, 512, 1, 0, 3) \
    MAUA_CONV_BOTH(X, 64, 128, 2, 0, 1) MAUA_CONV_BOTH(X, 64, 128, 2, 0, 2)
namespace {
const ConvInstance kConvInstances[] = {
    MAUA_CONV_ROWS(MAUA_CONV_ENTRY)
#ifdef MAUA_EXPERIMENTS
    MAUA_CONV_ROWS_EXPERIMENTS(MAUA_CONV_ENTRY)
#endif
};
}  // namespace
ConvTable maua_conv_table_m0() { return {kConvInstances, (int)(sizeof(kConvInstances) / sizeof(kConvInstances[0]))}; }
