// TEST INFRASTRUCTURE ONLY.  The product's host encoder (hypersonic_rans_amd/csrc/hsrans_host.cpp) built with
// HSRANS_KEEP_SHORT_LAST_BLOCK: the reference's block policy without the product's one deviation (a last block shorter than
// S symbols is left as it is), so that tests/oracle_lib.py can rebuild the reference's streams at those lengths.  Every stream
// it returns is checked there against the reference's recorded SHA-256 (tests/golden/reference_calls.json).
#include "../hypersonic_rans_amd/csrc/hsrans_host.h"

extern "C" size_t orc_refsplit_encode(int container, int states, unsigned bits, const uint8_t *in, size_t n, uint8_t *out, size_t cap)
{
  return hsrans::encode(container, states, bits, in, n, out, cap, nullptr, nullptr);
}
