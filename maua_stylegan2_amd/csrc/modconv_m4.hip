// Instances of modconv_mfma_kernel for mode 4, transposed with F(2,2) on the even x-phase.
#include "modconv_kernel.h"

#define MAUA_CONV_ROWS(X)                                                                          \
    X(32, 128, 1, 4, false, 3) X(64, 64, 2, 4, false, 2)                      /* transposed + F(2,2): flat runs only */
namespace {
const ConvInstance kConvInstances[] = {MAUA_CONV_ROWS(MAUA_CONV_ENTRY)};
}  // namespace
ConvTable maua_conv_table_m4() { return {kConvInstances, (int)(sizeof(kConvInstances) / sizeof(kConvInstances[0]))}; }
