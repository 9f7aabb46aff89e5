// TEST INFRASTRUCTURE ONLY: the host policies of the speculative scheduler (csrc/pma_epoch_policy.h) behind a few C entry points,
// as a library of its own (tests/hostsim/libpolicy_host.so): tests/test_epoch_policy.py drives the rules without a batch.
#include <string.h>

#include "pma_epoch_policy.h"

#define PH_API extern "C" __attribute__((visibility("default")))

using ppcsr::EpochPolicy;

PH_API EpochPolicy *policy_new() { return new EpochPolicy(); }
PH_API void policy_free(EpochPolicy *p) { delete p; }
// knobs by name (1: known)
PH_API int policy_set(EpochPolicy *p, const char *knob, uint32_t v) {
  uint32_t *f = !strcmp(knob, "epoch_ops") ? &p->epoch_ops : !strcmp(knob, "epoch_short") ? &p->epoch_short
              : !strcmp(knob, "epoch_grow_after") ? &p->epoch_grow_after : !strcmp(knob, "epoch_adapt") ? &p->epoch_adapt
              : !strcmp(knob, "region_slots") ? &p->region_slots : !strcmp(knob, "region_wide") ? &p->region_wide
              : !strcmp(knob, "region_calm") ? &p->region_calm : !strcmp(knob, "region_rare") ? &p->region_rare
              : !strcmp(knob, "region_rare_calm") ? &p->region_rare_calm : !strcmp(knob, "region_rare_dist") ? &p->region_rare_dist
              : !strcmp(knob, "region_rare_cpr") ? &p->region_rare_cpr : !strcmp(knob, "region_eff") ? &p->region_eff : nullptr;
  if (f) *f = v;
  return f ? 1 : 0;
}
PH_API void policy_set_since_rollback(EpochPolicy *p, uint64_t v) { p->since_rollback = v; }
PH_API void policy_begin_batch(EpochPolicy *p) { p->begin_batch(); }
PH_API int policy_region_shift(EpochPolicy *p, int logN) { return p->region_shift(logN); }
PH_API void policy_after_rollback(EpochPolicy *p) { p->after_rollback(); }
PH_API void policy_after_clean_epoch(EpochPolicy *p, uint64_t updates, uint64_t committed, uint64_t rounds) {
  p->after_clean_epoch(updates, committed, rounds);
}
// the state: u[] = epoch length, epoch_clean, grow_eff, region_eff, region_clean, since_rollback, region_rare_span, rare rule on;
// d[] = rb_dist, cpr_mean
PH_API void policy_state(const EpochPolicy *p, uint64_t *u, double *d) {
  const uint64_t s[8] = {p->epoch_len(), p->epoch_clean, p->grow_eff, p->region_eff, p->region_clean, p->since_rollback,
                         p->region_rare_span, p->rare_rule_on() ? 1u : 0u};
  memcpy(u, s, sizeof(s));
  d[0] = p->rb_dist;
  d[1] = p->cpr_mean;
}

PH_API uint32_t policy_chunk_grid(uint32_t opt_horizon, uint32_t width, uint64_t pending, uint64_t carry) {
  return ppcsr::chunk_grid(opt_horizon, width, pending, carry);
}
// rounds of the next chunk of an epoch opened at `width0` x `updates`, `cooldown` chunks after an exclusive update
PH_API uint32_t policy_chunk_rounds(uint32_t width0, uint64_t updates, uint32_t rounds_per_sync, uint32_t cooldown) {
  ppcsr::ChunkPlan ch;
  ch.open_epoch(width0, updates);
  ch.excl_cooldown = cooldown;
  return ch.next_rounds(rounds_per_sync);
}
// o_check choice: n chunks of (planned[i], long_checks[i]) more each (the engine passes the epoch's running totals); lanes[i] =
// the choice after chunk i
PH_API void policy_check_choice(const uint64_t *planned, const uint64_t *long_checks, int n, int *lanes) {
  ppcsr::CheckChoice c;
  c.open_epoch();
  unsigned long long P = 0, L = 0;
  for (int i = 0; i < n; i++) {
    P += planned[i];
    L += long_checks[i];
    c.after_chunk(P, L);
    lanes[i] = c.use_lanes() ? 1 : 0;
  }
}
// o_big choice: n chunks of (jobs[i], rounds[i]) more each; on[i] = the launch stays in after chunk i
PH_API void policy_big_choice(const uint64_t *jobs, const uint64_t *rounds, int n, int *on) {
  ppcsr::BigChoice b;
  b.open_epoch();
  unsigned long long J = 0, R = 0;
  for (int i = 0; i < n; i++) {
    J += jobs[i];
    R += rounds[i];
    b.after_chunk(J, R);
    on[i] = b.on ? 1 : 0;
  }
}
