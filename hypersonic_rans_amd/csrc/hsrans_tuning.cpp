// The one reader of the library's HSRANS_* switches (hsrans_tuning.h).
#include "hsrans_tuning.h"

#include <stdlib.h>

namespace hsrans
{

// up to n comma-separated decimal values of `s` into out; true when there were n (a longer list gives its first n)
static bool parse_list(const char *s, uint32_t *out, uint32_t n)
{
  uint32_t k = 0;
  for (const char *p = s; k < n && *p; k++)
  {
    out[k] = (uint32_t)strtoul(p, (char **)&p, 10);
    if (*p == ',')
      p++;
  }
  return k == n;
}

Tuning read_tuning()
{
  Tuning t;
  const char *e = nullptr;
  uint32_t v[10];
  auto set = [&](const char *name) { return (e = getenv(name)) != nullptr; };
  auto number = [&](const char *name, uint32_t *out) { if (set(name)) *out = (uint32_t)atoi(e); };
  auto unless_0 = [&](const char *name, bool *out) { if (set(name)) *out = atoi(e) != 0; };
  auto list = [&](const char *name, uint32_t n) { return set(name) && parse_list(e, v, n); };
  // a list of 8 class lengths inside the domain (hsrans_tuning.h: kClassLengthMin .. kClassLengthMax each); any other list is ignored as a whole
  auto class_list = [&](const char *name) {
    if (!list(name, 8))
      return false;
    for (uint32_t k = 0; k < 8; k++)
      if (v[k] < kClassLengthMin || v[k] > kClassLengthMax)
        return false;
    return true;
  };
  auto weights = [&](const char *name, uint32_t *w) { // ... rescaled to a sum of 8000 (rounded down: never above it)
    if (!class_list(name))
      return false;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < 8; k++)
      sum += v[k];
    for (uint32_t k = 0; k < 8; k++)
      w[k] = (uint32_t)((uint64_t)v[k] * 8000 / sum);
    return true;
  };
  t.waves_per_wg_set = set("HSRANS_WAVES_PER_WG");
  if (t.waves_per_wg_set && atoi(e) >= 4 && atoi(e) <= 16)
    t.waves_per_wg = (uint32_t)atoi(e);
  unless_0("HSRANS_SPREAD", &t.spread);
  weights("HSRANS_SLOT_WEIGHTS", t.slot_weights);
  weights("HSRANS_SLOT_WEIGHTS4", t.slot_weights4);
  t.direct_weights_set = weights("HSRANS_DIRECT_WEIGHTS", t.direct_weights);
  weights("HSRANS_DIRECT_WEIGHTS4", t.direct_weights4);
  weights("HSRANS_DIRECT_WEIGHTS6", t.direct_weights6);
  weights("HSRANS_DIRECT_WEIGHTS3", t.direct_weights3);
  weights("HSRANS_DIRECT_WEIGHTS_PAIR", t.direct_weights_pair);
  number("HSRANS_PRIVATE_PAIR", &t.private_pair);
  number("HSRANS_SINGLE_FAST", &t.single_fast);
  number("HSRANS_DUAL", &t.dual);
  weights("HSRANS_DUAL_WEIGHTS", t.dual_weights);
  weights("HSRANS_DUAL_WEIGHTS_WIDE", t.dual_weights_wide);
  t.table_spill = set("HSRANS_TABLE_SPILL") && e[0] != '\0' && e[0] != '0';

  number("HSRANS_GROUP_PRIO", &t.group_prio);
  if (list("HSRANS_GROUP_PRIO_CLASS", 10))
    for (uint32_t k = 0; k < 10; k++)
      t.group_prio_class[k] = (uint16_t)(v[k] > 1000 ? 1000 : v[k]);
  t.group_static = set("HSRANS_GROUP_STATIC");
  number("HSRANS_DEALT", &t.dealt);
  unless_0("HSRANS_DEALT_WIDE", &t.dealt_wide);
  if (set("HSRANS_DEALT_MIN_CHAINS") && atoi(e) > 0)
    t.dealt_min_chains = (uint32_t)atoi(e);
  if ((t.dealt_weights_set = class_list("HSRANS_DEALT_WEIGHTS"))) // (as given: not rescaled)
    for (uint32_t k = 0; k < 8; k++)
      t.dealt_weights[k] = v[k];
  number("HSRANS_DEALT_WT", &t.dealt_wt);
  if (set("HSRANS_DEALT_GAP_GROUPS"))
    t.dealt_gap_groups = (uint64_t)atoi(e);
  t.dealt_trace = set("HSRANS_DEALT_TRACE");

  if ((t.batch_weights_set = class_list("HSRANS_BATCH_WEIGHTS"))) // (as given: not rescaled)
    for (uint32_t k = 0; k < 8; k++)
      t.batch_weights[k] = v[k];
  t.batch_stamps = set("HSRANS_BATCH_STAMPS");
  unless_0("HSRANS_SHARD_ONE_LAUNCH", &t.shard_one_launch);
  t.calibrate = set("HSRANS_CALIBRATE") && atoi(e) != 0;
  t.hip_strict = set("HSRANS_HIP_STRICT") && e[0] != '\0' && e[0] != '0';
  t.host_index_cache_off = set("HSRANS_HOST_INDEX_CACHE_OFF");
  t.index_assemble_on_host = set("HSRANS_INDEX_ASSEMBLE_ON_HOST");
  t.hpipe_direct = set("HSRANS_HPIPE_DIRECT");
  t.debug_stamps = set("HSRANS_DEBUG_STAMPS");
  t.hpipe_trace = set("HSRANS_HPIPE_TRACE");
  t.indexing_trace = set("HSRANS_INDEXING_TRACE");
  if (set("HSRANS_GATHER_MIN_SEGMENT") && atoi(e) >= 64 && atoi(e) <= (1 << 30))
    t.gather_min_segment = (uint32_t)atoi(e);
  return t;
}

} // namespace hsrans
