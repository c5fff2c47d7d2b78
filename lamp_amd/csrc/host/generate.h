// lamp.data.languagemodel.autoregressiveInference (lamp-data/src/main/scala/lamp/data/languagemodel/package.scala:35-114) over a
// LanguageModelModule: the reference's chain, or one row per block against a key / value cache (kernels/decode.hip).  DESIGN.md section 18.
#pragma once
#include "transformer.h"

namespace lamp {
namespace host {

constexpr bool kDecodeFusedDefault = true;   // BASELINE.md section 16 holds the measurement behind it
bool decode_fused();
bool set_decode_fused(bool on);   // returns the previous value
int last_generate_path();         // 1 the decode kernels, 0 the chain, -1 no call yet

struct Generated { Ten tokens, logits; };   // [B, P + length] int64; [B, length, V] (undefined unless asked for)
Generated language_model_generate(LanguageModelModule& lm, const Ten& prefix, int64_t length, double temperature, int64_t modelBlockSize,
                                  bool wantLogits);

}  // namespace host
}  // namespace lamp
