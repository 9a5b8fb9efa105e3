// Host-side planning of the window joint histogram (window_joint.h): which ring a pair
// lives in, which lane of a row counts it, and how a window and its pieces are cut. No HIP
// in here: the kernel (window_joint.hip) and a host-only check under sanitizers
// (tools/joint_plan_check.cpp) compile the same text.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ROCMDASH_JOINT_HD __host__ __device__
#else
#define ROCMDASH_JOINT_HD
#endif

namespace rocmdash {

constexpr uint32_t kMaxJointPairs = 8;
constexpr uint32_t kMaxJointBuckets = 31;  // (B + 1)^2 <= 1024 cells per pair
constexpr uint32_t kMaxJointStride = 64;   // floats per ring row: a wave holds at least one row
constexpr uint32_t kJointOwnerPasses = 2;  // a lane of a row owns at most this many pairs

// ---- owners ------------------------------------------------------------------------------
// The lanes of a wave hold rows of `stride` lanes each; lane c of a row (c = lane % stride,
// a series or a padding column alike) owns the ring's distinct pair q = pass * stride + c,
// in pass 0 and pass 1. A ring has at most min(8, stride x (stride - 1)) distinct ordered
// pairs, which is at most 2 x stride for every stride >= 2: two passes always do.
ROCMDASH_JOINT_HD inline int joint_owned_pair(uint32_t stride, uint32_t distinct, uint32_t c, uint32_t pass) {
  const uint32_t q = pass * stride + c;
  return (c < stride && pass < kJointOwnerPasses && q < distinct) ? int(q) : -1;
}
// byte q of a packed word (q < 8)
ROCMDASH_JOINT_HD inline uint32_t joint_byte(uint64_t packed, uint32_t q) { return uint32_t(packed >> (8u * q)) & 0xffu; }

// ---- pairs onto rings --------------------------------------------------------------------
struct JointRingSpan {
  uint32_t first_series, width;  // the ring's series are [first_series, first_series + width)
};

// The pairs of one ring, as the kernel takes them: its `distinct` ordered pairs (columns of
// the ring, a byte each, packed) and per distinct pair the set of output slots k (a bit each)
// that asked for it - a pair named twice is counted once and added to both slots.
struct JointRingPairs {
  uint32_t ring = 0, distinct = 0;
  uint64_t a = 0, b = 0, slots = 0;
};

struct JointPlan {
  JointRingPairs rings[kMaxJointPairs];  // only rings with pairs, in ring order
  uint32_t nrings = 0;
};

// pairs: [K][2] series indices of the set. False - nothing usable in *plan - unless
// 1 <= K <= 8 and every pair has a != b, both below the set's series and both in one ring.
inline bool joint_plan_pairs(const uint32_t* pairs, uint32_t K, const JointRingSpan* spans, uint32_t nspans,
                             JointPlan* plan) {
  *plan = JointPlan{};
  if (pairs == nullptr || K < 1 || K > kMaxJointPairs) return false;
  int32_t ring_of[kMaxJointPairs];
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t a = pairs[2 * k], b = pairs[2 * k + 1];
    if (a == b) return false;
    int32_t ra = -1, rb = -1;
    for (uint32_t r = 0; r < nspans; ++r) {
      if (a >= spans[r].first_series && a - spans[r].first_series < spans[r].width) ra = int32_t(r);
      if (b >= spans[r].first_series && b - spans[r].first_series < spans[r].width) rb = int32_t(r);
    }
    if (ra < 0 || rb < 0 || ra != rb) return false;  // beyond the set, or a pair across rings
    if (spans[ra].width > kMaxJointStride) return false;
    ring_of[k] = ra;
  }
  for (uint32_t r = 0; r < nspans; ++r) {
    JointRingPairs p;
    p.ring = r;
    for (uint32_t k = 0; k < K; ++k) {
      if (ring_of[k] != int32_t(r)) continue;
      const uint32_t a = pairs[2 * k] - spans[r].first_series, b = pairs[2 * k + 1] - spans[r].first_series;
      uint32_t q = 0;
      while (q < p.distinct && !(joint_byte(p.a, q) == a && joint_byte(p.b, q) == b)) ++q;
      if (q == p.distinct) {
        p.a |= uint64_t(a) << (8u * q);
        p.b |= uint64_t(b) << (8u * q);
        ++p.distinct;
      }
      p.slots |= uint64_t(1u << k) << (8u * q);
    }
    if (p.distinct) plan->rings[plan->nrings++] = p;
  }
  return true;
}

// ---- blocks and pieces -------------------------------------------------------------------
// The window [head - rows, head) of a ring of `depth` rows (a power of two), rows <= depth,
// rows <= head: one contiguous block of slots, or two when it wraps - [first, first + tail),
// then [0, rows - tail).
struct JointCut {
  uint64_t first = 0, tail = 0, rest = 0;
};
inline JointCut joint_cut(uint64_t depth, uint64_t head, uint64_t rows) {
  JointCut c;
  if (rows == 0) return c;
  c.first = (head - rows) & (depth - 1);
  c.tail = rows < depth - c.first ? rows : depth - c.first;
  c.rest = rows - c.tail;
  return c;
}

// A block of `floats` = rows x stride floats is cut into pieces of L = (64 / stride) x
// stride floats - whole rows, so lane l stays on series l % stride - and workgroup g of
// `groups` takes the pieces [g x share, min((g + 1) x share, pieces)).
ROCMDASH_JOINT_HD inline uint32_t joint_piece_floats(uint32_t stride) { return 64u / stride * stride; }
ROCMDASH_JOINT_HD inline uint32_t joint_pieces(uint64_t floats, uint32_t stride) {
  const uint32_t L = joint_piece_floats(stride);
  return uint32_t((floats + L - 1) / L);
}
ROCMDASH_JOINT_HD inline uint32_t joint_share(uint32_t pieces, uint32_t groups) { return (pieces + groups - 1) / groups; }

}  // namespace rocmdash
