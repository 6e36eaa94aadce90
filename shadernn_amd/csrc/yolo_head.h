// yolo_head.h -- the constants the YOLO head kernel (yolo_head.hip) and its plan share.
#pragma once

namespace snnhip {

constexpr int kYoloHeadThreads = 256;         // one block per image
constexpr int kYoloHeadMaxCandidates = 4096;  // keys: 32 KiB, one lane of wave 0 per 64-bit mask word
constexpr int kYoloHeadMaxAnchors = 3;        // per cell: masks[6] serves two heads
constexpr int kYoloHeadMaxClasses = 1 << 20;  // the class rides in the 20 bits below the candidate index of a sort key

// the instance of a plan: the smallest table that holds every candidate of an image
constexpr int yolo_head_capacity(int candidates) { return candidates <= 256 ? 256 : candidates <= 1024 ? 1024 : 4096; }
// static LDS of that instance: keys (8 bytes), boxes (16 bytes), one bit of the merged mask per position, the two block counters
constexpr int yolo_head_lds_bytes(int cap) { return cap * (8 + 16) + cap / 8 + 8; }

} // namespace snnhip
