// The rule for a caller's list of checkpoint groups (hsrans_encode_opts::index_groups, hsrans_index_build_at and their device and host
// twins): every group non-zero, a multiple of 4 (a set boundary) and above the one before.  Plain C++: hsrans_cpu.cpp is no HIP unit.
#ifndef HSRANS_INDEX_GROUPS_H
#define HSRANS_INDEX_GROUPS_H

#include <stddef.h>
#include <stdint.h>

namespace hsrans
{

inline bool index_groups_valid(const uint64_t *groups, size_t n)
{
  for (size_t k = 0; k < n; k++)
    if (groups[k] == 0 || (groups[k] % 4) != 0 || (k > 0 && groups[k] <= groups[k - 1]))
      return false;
  return true;
}

} // namespace hsrans

#endif // HSRANS_INDEX_GROUPS_H
