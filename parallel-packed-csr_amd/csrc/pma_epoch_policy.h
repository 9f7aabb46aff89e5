// Host policies of the speculative scheduler (Engine::run_speculative): how long the next epoch is, how wide the regions of the
// per-region prefix rule are, and the per-chunk decisions between two looks at the device's control block.  Plain host
// arithmetic: nothing here knows the runtime or the kernels, so the rules can be driven from a test without a batch
// (tests/hostsim/policy_host.cpp).  Built with -ffp-contract=off like the library: the running means are fp64.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace ppcsr {

struct EpochPolicy {
  // ---- knobs (Engine::set_option writes them) ----
  uint32_t epoch_ops = 1u << 20;  // rollback granularity (upper bound)
  // (a snapshot costs about one round; a rollback re-does half an epoch on average.  On a config #4 partition — 3 rollbacks
  // per 1.25 M inserts — 8192 / 8 spent 16 % of the batch copying snapshots: 16384 / 2 took 30.4 ms instead of 38.4; the
  // Zipf stream on the same partition, 50 rollbacks per 1.5 M updates, was indifferent: 208 ms either way)
  uint32_t epoch_short = 16384;    // epoch length after a rollback
  uint32_t epoch_grow_after = 2;   // how many clean epochs in a row double the length again
  // Round 3: with incremental snapshots an epoch boundary costs ~30 us, so a stream that rolls back often is better off with
  // epochs a good deal shorter than the distance between its rollbacks (hot-vertex stream: one rollback per 28 K updates;
  // 2048-update epochs that double after 4 clean ones: 121 -> 105 ms per 1 M), while a stream that rolls back three times
  // per million (a config #4 partition) needs the long ones (4096-update epochs: 24 -> 35 ms).  epoch_adapt = 1: the epoch
  // after a rollback is 1/epoch_adapt (default 8) of the running mean distance between rollbacks, within [2048, epoch_short].
  uint32_t epoch_adapt = 8;  // (0 off, else the divisor)
  // per-region prefix rule: nothing later may commit in a region where an earlier update was deferred.  4096 slots blocked
  // 43 K of the 69 K non-commits per 1 M updates of config #2 for nothing (179 M/s; 2048: 184, 1024: 187, 512: 188, 256: 189);
  // the hot-vertex stream needs the rule (1024: 142 ms as with 4096, 83 rollbacks instead of 36; 256: 191 ms, 199 rollbacks)
  uint32_t region_slots = 1024;
  // ... so the rule is tightened where rollbacks happen: after one, regions are region_wide slots until region_calm epochs in
  // a row have ended cleanly (a config #4 partition at critical density: 31.1 ms / 9 rollbacks with 1024 throughout, 26.7 ms
  // / 3 rollbacks with 4096; its calm second half is config-#2-like again)
  uint32_t region_wide = 4096, region_calm = 8;
  // Round 3: a stream whose rollbacks are RARE (running mean distance >= region_rare_dist updates: a config #4 partition at
  // critical density, one per ~150 K updates while its levels sit at their bounds) is better off paying for none at all:
  // region_rare slots after a rollback, for region_rare_calm (8) x that distance of committed updates (24.9 -> 19.3 ms per batch of
  // the partition: 193 -> 157 rounds, 0 rollbacks; the wide rule ends about where the array doubles and the stream turns calm).
  // A stream that rolls back all the time (hot vertices, one per 28 K updates) keeps region_wide / region_calm: with 16 K-slot
  // regions it loses more commits per round than the rollbacks cost (105 -> 131 ms); a stream that never rolls back never
  // sees either rule.
  uint32_t region_rare = 16384, region_rare_calm = 8, region_rare_dist = 65536;
  // ... and only for streams that commit a good share of a chip-full per round (running mean >= region_rare_cpr): wide regions
  // make rollbacks rarer for ANY stream, so the distance alone would also switch the rule on for the hot-vertex stream once it
  // has been on for a while (600-750 commits per round there, 6-8 K on the critical-density partition)
  uint32_t region_rare_cpr = 1536;

  // ---- state (lives as long as the engine: a batch takes up where the last one stopped) ----
  // adaptive epoch length: a rollback throws away everything since the epoch's snapshot, so a stream that provokes
  // rollbacks (hot vertices whose windows balloon while they wait) is cut into short epochs — epoch_short updates after a
  // rollback, doubling again with every epoch that ends cleanly — while a stream that never rolls back keeps one
  // snapshot per epoch_ops updates
  uint32_t cur_epoch = 0;
  uint32_t epoch_clean = 0;  // clean epochs in a row
  uint32_t grow_eff = 2;     // how many of them double the length (epoch_grow_after, or 4 after a shortened epoch)
  uint64_t since_rollback = 0;
  double rb_dist = -1.0;     // running mean distance between rollbacks, updates (< 0: none seen yet)
  uint32_t region_eff = 0, region_clean = 0;  // the region width in force (0: region_slots, not looked at yet) / clean epochs under a wide one
  uint64_t region_rare_span = 0;  // > 0: the rare rule is on until this many updates have committed since the rollback
  double cpr_mean = -1.0;         // running mean of commits per round over the clean epochs (< 0: none yet)

  void begin_batch() { if (cur_epoch == 0 || cur_epoch > epoch_ops) cur_epoch = epoch_ops; }
  uint32_t epoch_len() const { return cur_epoch; }
  // OptArgs::regshift of an epoch on an array of 2^logN slots (brings region_eff up to region_slots first)
  int region_shift(int logN) {
    int rs = 0;
    if (region_eff < region_slots) region_eff = region_slots;
    while ((region_eff >> rs) > (uint32_t)logN) rs++;
    return rs;
  }
  // the rare-rollback rule keeps the regions wide
  bool rare_rule_on() const { return region_rare_span && region_eff >= region_rare; }

  void after_rollback() {
    uint32_t short_eff = epoch_short;
    grow_eff = epoch_grow_after;
    if (epoch_adapt) {
      const double D = (double)std::min<uint64_t>(since_rollback, 64ull * epoch_short);
      // (running mean with a fast attack downwards: a stream that starts to roll back often is recognised at once)
      rb_dist = rb_dist < 0 ? 64.0 * epoch_short : (D < rb_dist ? 0.25 * rb_dist + 0.75 * D : 0.5 * rb_dist + 0.5 * D);
      since_rollback = 0;
      uint32_t q = 2048;
      while (2ull * q <= (uint64_t)(rb_dist / (double)epoch_adapt) && 2ull * q <= epoch_short) q *= 2;
      short_eff = std::min<uint32_t>(epoch_short, q);
      if (short_eff < epoch_short) grow_eff = std::max<uint32_t>(epoch_grow_after, 4u);
    }
    cur_epoch = std::min<uint32_t>(cur_epoch, std::min<uint32_t>(epoch_ops, short_eff));
    epoch_clean = 0;
    const bool rare = epoch_adapt && region_rare && rb_dist >= (double)region_rare_dist && cpr_mean >= (double)region_rare_cpr;
    region_eff = std::max(region_slots, rare ? std::max(region_wide, region_rare) : region_wide);
    region_rare_span = rare ? (uint64_t)(region_rare_calm * rb_dist) : 0;
    region_clean = 0;
  }

  // an epoch of `updates` updates ended without a rollback: `committed` of them in `rounds` rounds
  void after_clean_epoch(uint64_t updates, unsigned long long committed, unsigned long long rounds) {
    since_rollback += updates;
    if (rounds) {
      const double cpr = (double)committed / (double)rounds;
      cpr_mean = cpr_mean < 0 ? cpr : 0.75 * cpr_mean + 0.25 * cpr;
    }
    if (region_eff != region_slots) {
      ++region_clean;
      if (region_rare_span ? since_rollback >= region_rare_span : region_clean >= region_calm) {
        region_eff = region_slots;
        region_rare_span = 0;
      }
    }
    if (++epoch_clean >= std::max(grow_eff, epoch_grow_after)) {
      cur_epoch = (uint32_t)std::min<uint64_t>(epoch_ops, 2ull * cur_epoch);
      epoch_clean = 0;
    }
  }
};

// ---- chunk-level decisions: a chunk is the rounds launched between two reads of the control block ----

// grid of a chunk: wide enough for the adapted width to grow during the chunk (x1.25 per full-width round), narrow at the
// tail, never narrower than the carry list (a round plans the whole of it) and never wider than opt_horizon
inline uint32_t chunk_grid(uint32_t opt_horizon, uint32_t width, uint64_t pending, uint64_t carry) {
  uint32_t gh = opt_horizon;
  const uint64_t want = std::max<uint64_t>(1024, 4ull * (width ? width : opt_horizon));
  if (want < gh) gh = (uint32_t)want;
  const uint64_t pend = (pending + 255) & ~255ull;
  if (pend < gh) gh = (uint32_t)std::max<uint64_t>(pend, 256);
  const uint64_t need = (carry + 255) & ~255ull;
  if (gh < need) gh = (uint32_t)std::min<uint64_t>(need, opt_horizon);
  return gh;
}

// where the chunks of one epoch stand: what the device last reported and the tail sizing that follows from it
struct ChunkPlan {
  uint32_t width = 0;    // the adapted width the device last reported
  uint64_t carry = 0;    // deferred updates waiting in the carry list
  uint64_t pending = 0;  // updates still pending: the carry list and the fresh ones
  double cpr = 0;        // updates committed per round (measured on the last chunk)
  unsigned long long prev_rounds = 0, prev_committed = 0;
  uint32_t excl_cooldown = 0;  // chunks to keep short after an exclusive update (the launches behind it in its chunk are wasted)

  void open_epoch(uint32_t width0, uint64_t updates) {
    *this = ChunkPlan();
    width = width0;
    pending = updates;
    cpr = 0.9 * (double)std::min<uint64_t>(width0, updates);
  }
  void resume(uint32_t width_now, uint64_t carried, uint64_t fresh) {
    width = width_now;
    carry = carried;
    pending = carried + fresh;
  }
  // the epoch's counters after a chunk that ended on nothing special
  void measured(unsigned long long rounds, unsigned long long committed) {
    if (rounds > prev_rounds) cpr = (double)(committed - prev_committed) / (double)(rounds - prev_rounds);
    prev_rounds = rounds;
    prev_committed = committed;
  }
  // rounds in the next chunk: as many as rounds_per_sync while that many are needed, fewer at the tail of the epoch so
  // that the stream is not padded with launches that find `done` set (each still costs ~2 us of dispatch)
  uint32_t next_rounds(uint32_t rounds_per_sync) {
    uint32_t rounds = rounds_per_sync;
    const double per_round = std::max(1.0, 0.85 * cpr);
    const double est = (double)pending / per_round + 2.0;
    if (est < (double)rounds) rounds = (uint32_t)std::max(2.0, est);
    if (excl_cooldown) {
      rounds = std::min<uint32_t>(rounds, 8u);
      excl_cooldown--;
    }
    return rounds;
  }
};

// o_check: a lane per update while updates have short footprints (one leaf, two or three read ranges); a wave per update for
// streams where more than ~1 in 64 has a long one (hot ranges, critical density: big windows, many-level climbs, runs of moved
// sentinels), which the lane kernel leaves to its wave one by one
struct CheckChoice {
  bool lanes = true;
  uint32_t wave_chunks = 0;
  int force = -1;  // option "check_lanes": -1 by the share of long footprints (default), 0 always a wave per update, 1 always a lane
  unsigned long long planned_seen = 0, long_seen = 0;  // the epoch's counters at the last look

  void open_epoch() { planned_seen = long_seen = 0; }
  bool use_lanes() const { return force >= 0 ? force == 1 : lanes; }
  // which o_check for the next chunk.  The lane kernel counts what it had to leave to the wave (each such update costs its wave
  // a serial ~5 us): above ~1 in 64 a wave per update from the start is faster.  From the wave kernel the way back is a trial
  // chunk every so often.
  void after_chunk(unsigned long long planned, unsigned long long long_checks) {
    const unsigned long long dp = planned - planned_seen, dl = long_checks - long_seen;
    planned_seen = planned;
    long_seen = long_checks;
    if (lanes) {
      if (dp >= 1024 && dl * 64ull > dp) {
        lanes = false;
        wave_chunks = 0;
      }
    } else if (++wave_chunks >= 24u) {
      lanes = true;
    }
  }
};

// o_big (the launch that rebalances the windows a round queues for workgroups) is left out of the rounds while a stream queues
// none: a round that does queue one then stops the chunk (OptCtl::need_big), the host runs the launch and keeps it in for a while
struct BigChoice {
  bool on = false;
  double rate = 0;  // queued windows per round, running mean
  unsigned long long jobs_seen = 0, rounds_seen = 0;  // the epoch's counters at the last look

  void open_epoch() { jobs_seen = rounds_seen = 0; }
  // keep / drop the launch: kept while a stream queues a window every few rounds (an empty launch costs ~4 us, a round that
  // finds none where it needs one costs the rest of its chunk)
  void after_chunk(unsigned long long jobs_total, unsigned long long rounds) {
    const unsigned long long dj = jobs_total - jobs_seen, dr = rounds - rounds_seen;
    jobs_seen = jobs_total;
    rounds_seen = rounds;
    if (dr) rate = 0.5 * rate + 0.5 * (double)dj / (double)dr;
    on = rate >= 1.0 / 12.0;
  }
};

}  // namespace ppcsr
