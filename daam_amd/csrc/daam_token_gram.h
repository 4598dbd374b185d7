// daam_token_gram (include/daam_analysis.h) between its kernels and its host entry point (both in daam_token_gram.hip):
// the decomposition's constants and the launch descriptor.  The keys' sizes live on the device, so the host sizes the launch from
// n_keys, n_rows and the scratch it was given alone: grid = n_keys x cap chunks, and a workgroup past its key's last chunk exits.
#pragma once
#include "daam_key_planes.h"

namespace daam {

constexpr int kGramThreads = 256;                // four waves: each takes a quarter of every sub-tile's k-steps
constexpr int kGramChunk = 1024;                 // pixels of a workgroup: a function of nothing but the kernel
constexpr int kGramSub16 = 128;                  // pixels of a staged sub-tile, 16-bit path: 8 k-steps of 16
constexpr int kGramSub32 = 64;                   // ... f32 path: 32 k-steps of 2
constexpr int kGramRow16 = kGramSub16 * 2 + 16;  // LDS bytes of a staged row, 16-bit path: 16 lanes' 16-byte reads cover every bank
constexpr int kGramRow32 = kGramSub32 + 1;       // LDS floats of a staged row, f32 path
constexpr int kGramRed = 16 * 65;                // floats of one wave's 32 x 32 block in the join: register g at g * 65 + lane
constexpr int kGramMaxRows = 96;
constexpr int kGramMaxChunks = kKeyMaxSide * kKeyMaxSide / kGramChunk;

struct GramLaunch {
    const DaamKeyPlanes* keys;
    float* gram;                                 // [n_keys][n_rows][n_rows]
    float* scratch;                              // [n_keys][cap][n_rows][n_rows]: the chunks' matrices of keys of more than one
    int32_t n_keys, n_rows;
    int32_t cap;                                 // chunks per key the scratch holds, 1 .. kGramMaxChunks
    int32_t multi_only;                          // the f32-path launch beside a 16-bit one: only valid keys with n_win > 1
};

__host__ __device__ inline int gram_chunks(int hw) { return (hw + kGramChunk - 1) / kGramChunk; }

}  // namespace daam
