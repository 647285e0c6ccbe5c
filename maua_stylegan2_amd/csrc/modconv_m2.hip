// Instances of modconv_mfma_kernel for mode 2, Winograd F(2,3) along x.
#include "modconv_kernel.h"

#define MAUA_CONV_ROWS(X)                                                                          \
    MAUA_CONV_BOTH(X, 128, 64, 2, 2, 1) MAUA_CONV_BOTH(X, 128, 64, 2, 2, 2)   /* F(2,3) */         \
    MAUA_CONV_BOTH(X, 64, 128, 1, 2, 2)                                                            \
    MAUA_CONV_BOTH(X, 32, 128, 1, 2, 2)
// The tile config only the A/B bits of an experiments build select (g_conv_cfg), with every MULTI x MAXP its patch limit allows.
#define MAUA_CONV_ROWS_EXPERIMENTS(X) \
    MAUA_CONV_BOTH(X, 32, 256, 1, 2, 1) MAUA_CONV_BOTH(X, 32, 256, 1, 2, 2) MAUA_CONV_BOTH(X, 32, 256, 1, 2, 3)
namespace {
const ConvInstance kConvInstances[] = {
    MAUA_CONV_ROWS(MAUA_CONV_ENTRY)
#ifdef MAUA_EXPERIMENTS
    MAUA_CONV_ROWS_EXPERIMENTS(MAUA_CONV_ENTRY)
#endif
};
}  // namespace
ConvTable maua_conv_table_m2() { return {kConvInstances, (int)(sizeof(kConvInstances) / sizeof(kConvInstances[0]))}; }
