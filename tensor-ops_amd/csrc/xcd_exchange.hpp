// The tagged exchange between the workgroups of a persistent kernel through ONE XCD's L2, stated once: online_sgd.hip,
// induce_seq.hip, ae_online.hip and rnn_wide.hip keep parameters in LDS for a whole call and pass small vectors to each
// other with what is here.  Their own headers describe their partitions only.
//
// Precondition: one L2.  Every participating workgroup sits on one XCD: the grid is 8 G workgroups, workgroup b runs on XCD
//   b % 8, and a kernel keeps the workgroups of one residue (xcd_placement_ok() probes that the dispatcher really places
//   them so; the callers ask before they take such a route).  All accesses to the exchange are relaxed, agent-scope, L1-
//   bypassing atomics: readers and writers meet in that one L2, with no device-scope write-back or invalidate (which is what
//   made a cross-XCD grid barrier cost 180 us).  online_sgd, induce_seq and ae_online are only RIGHT under this
//   placement; for rnn_wide it is a performance precondition.  Residency of the G workgroups comes from the grid size alone
//   (8 G <= 256 workgroups, one per CU).
//
// Publish and poll.  Every 32-bit word of a value travels with tag = step + 1 in ONE 64-bit store (publish); a reader
//   polls the words it needs until their tags say "this step" (poll), some in flight at a time, asking again only for those
//   that have not arrived.  Data and "it is there" are the same memory transaction: one L2 round trip a step (store -> L2 ->
//   load), where a counter barrier needs three (store ack, arrive, poll, then load).  The buffer is zero at launch, so no
//   tag of an earlier launch passes for one of this launch; a tag is 32 bits, so a launch has fewer than 2^32 - 1 steps.
//
// Two parity slots.  A step's words go to slot (step & 1) and a slot is rewritten two steps later.  That is safe: its
//   writer reaches the store of step s + 2 only after it has read EVERY peer's publication of step s + 1, and each peer
//   made that publication only after it had read all of step s -- this slot included.  So nobody can still be waiting to
//   read the word that is overwritten.
//
// The watchdog.  Every wait is bounded by watchdog_ticks() of wall_clock64 (TOPS_ONLINE_TIMEOUT_S, 2 s).  A workgroup whose
//   wait runs out reports the step in a host-visible status word and leaves; its peers then wait for a publication that
//   never comes and run out likewise, so a launch always ends.
//
// The single decision (kernels that write parameters back: online_sgd, ae_online).  A workgroup that got through its stream
//   votes "ok" and waits for the other votes.  Votes alone cannot make the write-back all-or-nothing: a peer that saw every
//   "ok" in time would write its slice while one whose poll timed out a moment earlier would not -- parameters half updated.
//   So the outcome is a single word that is decided exactly once, by compare-and-swap: whoever has seen all G "ok" votes
//   proposes COMMIT, whoever has seen a "failed" vote or run out of time proposes ABORT (give_up), the first proposal wins
//   and EVERYBODY obeys the word, not their own view.  A workgroup that timed out but reads COMMIT writes its slice after
//   all: COMMIT can only have been proposed by a peer that saw all G votes "ok", this one's included, so every slice is
//   complete.
//
// What is shared in code and what is not.  publish (four of its five sites), give_up, the vote block's constants and the
// host side below are shared.  The four poll loops, the two commits, rnn_wide's publish and induce_seq's dot product stay
// written out in their kernels, each with a line saying so: these kernels' assembly is held to the parent's bit for bit, and
// every shared form that was tried at a site changed that site's generated code (register allocation and scheduling, not
// arithmetic).  profiles/xcd_exchange_asm_identity.txt lists every form tried, site by site, with its digest -- a poll
// primitive with the flight count as a template parameter, "have" as a bool array or as a bit mask, an address functor or
// an index array, at each of the four sites; commit in six forms -- so that the next attempt starts from there (a
// compiler upgrade moves every digest anyway, and is the moment to share them).  They follow the contract above.
#pragma once
#include "common.hpp"

namespace to {
namespace xe {

// ---- device ---------------------------------------------------------------------------------------------------------------
// one value into its exchange slot: each 32-bit word with the step's tag in ONE 64-bit store
template <class S>
__device__ __forceinline__ void publish(unsigned long long* slot, S v, unsigned tag) {
  constexpr int WORDS = sizeof(S) / 4;
  unsigned wd[WORDS];
  __builtin_memcpy(wd, &v, sizeof(S));
#pragma unroll
  for (int u = 0; u < WORDS; ++u)
    __hip_atomic_store(slot + u, ((unsigned long long)tag << 32) | wd[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the vote block: 32 vote slots (one 64-bit word a workgroup), behind them the decision word
constexpr int DECISION = 32;
constexpr unsigned long long COMMIT = 1ull, ABORT = 2ull;
constexpr size_t VOTE_BYTES = 512;

// a peer never showed up: this workgroup votes "failed", decides ABORT for everybody (unless COMMIT was decided --
// impossible: that needs this vote to be "ok") and leaves
__device__ __forceinline__ void give_up(unsigned long long* votes, int g) {
  if (threadIdx.x == 0) {
    __hip_atomic_store(votes + g, 2ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long expect = 0ull;
    __hip_atomic_compare_exchange_strong(votes + DECISION, &expect, ABORT, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- host (xcd_exchange.hip) ------------------------------------------------------------------------------------------------
// What a kernel file keeps between launches, one instance a file: a grow-only exchange buffer, the vote block where the
// kernel commits, and 16 host-mapped bytes of status (the kernel's own type: int, or long long[2]).
struct XcdExchange {
  explicit XcdExchange(bool with_votes) : with_votes_(with_votes) {}
  void reserve(size_t bytes);    // the exchange holds at least `bytes`; the vote and status blocks exist
  void zero(hipStream_t s);      // the reserved bytes and the votes, in stream order
  void status_reset();           // "no report" (nothing of this instance is in flight)
  template <class T> T* status() const { return static_cast<T*>(status_); }          // the host's view; null before the first use
  template <class T> T* status_dev() const { return static_cast<T*>(status_dev_); }  // the kernel's
  unsigned long long* exch() const { return static_cast<unsigned long long*>(exch_); }
  unsigned long long* votes() const { return votes_; }

 private:
  void status_alloc();
  bool with_votes_;
  void* exch_ = nullptr;
  size_t cap_ = 0, used_ = 0;
  unsigned long long* votes_ = nullptr;
  void *status_ = nullptr, *status_dev_ = nullptr;
};

long long watchdog_ticks();   // TOPS_ONLINE_TIMEOUT_S (default 2 s) in wall_clock64 ticks, read once per process

// a kernel of these files may use all 160 KiB of LDS: the attribute, set once per kernel instantiation
constexpr int LDS_MAX = 160 * 1024;
template <auto Kern>
void allow_full_lds() {
  static bool done = false;
  if (done) return;
  TO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
  done = true;
}

}  // namespace xe
}  // namespace to
