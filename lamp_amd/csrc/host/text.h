// lamp.data.Text's generation over the recurrent family: sequencePrediction and sequencePredictionBeam (lamp-data/src/main/scala/lamp/data/
// Text.scala:18-135).  Values only.  A module of the shape Embedding -> RNN | GRU | LSTM -> [relu] -> SeqLinear -> [logSoftMax(2)] in f32 or
// f64 on a device with at most LAMP_DECODE_MAX_ROWS rows takes the fused path: the prefix once through the module's own forward, then per
// token lamp_recurrent_decode_step, lamp_decode_linear and lamp_log_softmax_argmax_rows (kernels/recurrent_decode.hip).
// Everything else takes the chain: FreeRunningRNN's loop, the reference's beam loop over the module's forward.
#pragma once
#include "recurrent.h"

namespace lamp {
namespace host {

constexpr bool kTextFusedDefault = true;
bool text_fused();
bool set_text_fused(bool on);   // returns the previous value
int last_text_path();           // 1 fused, 0 chain, -1 no call yet

struct Predicted { Ten tokens, outputs; };   // [steps, B] int64, [steps, B, V]
// FreeRunningRNN(module, steps).forward((prefix, module.initState)): the outputs' values and their argmax(2).  prefix: int64 [T0, B]
Predicted sequence_prediction(const Mod& module, const Ten& prefix, int64_t steps);

struct BeamResult { std::vector<int64_t> tokens; double logProb; };
// Text.scala:38-135 for one prefix [T0, 1]: the k best sequences, best first; each starts with the prefix's last token
std::vector<BeamResult> sequence_prediction_beam(const Mod& module, const Ten& prefix, int64_t steps, int64_t startSequence, int64_t endOfSequence,
                                                 int64_t k);

}  // namespace host
}  // namespace lamp
