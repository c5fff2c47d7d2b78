// lamp.nn's recurrent family over the C ABI: RNN, GRU, LSTM, SeqLinear, statefulSequence, FreeRunningRNN, Seq2Seq, WithInit.
//
// Reference: lamp-core/src/main/scala/lamp/nn/{RNN,GRU,LSTM,SeqLinear,StatefulSeq,FreeRunningRNN,Seq2Seq}.scala.  A cell is one autograd node over the
// whole sequence (F::lstm / F::gru / F::rnn): one GEMM for x.Wx + bias of all time steps, per step one GEMM for h.Wh and a fused cell
// kernel (kernels/recurrent.hip), backpropagation through time in the node's one shared backward.  With the switch off, for types
// other than f32 / f64 and for host tensors the same functions build the reference's fold out of the existing operators.
#pragma once
#include "nn.h"

namespace lamp {
namespace host {
namespace F {

struct SeqResult { Var out, h, c; };   // out [T, B, H], the last hidden state, the last memory (LSTM only)
// weights in the order of the module's `state`; h0 / c0 null = the reference's None (param(zeros))
SeqResult lstm(const Var& x, const std::vector<Var>& w, const Var& h0, const Var& c0);   // Xi Xf Xo Hi Hf Ho Xc Hc bI bF bO bC (LSTM.scala:28-42)
SeqResult gru(const Var& x, const std::vector<Var>& w, const Var& h0);                   // Xh Hh Xr Xz Hr Hz bR bZ bH (GRU.scala:27-38)
SeqResult rnn(const Var& x, const std::vector<Var>& w, const Var& h0);                   // Xh Hh bH (RNN.scala:20-25)
Var seq_linear(const Var& x, const Var& weight, const Var& bias);                        // SeqLinear.scala:22-29
// LossFunctions.SequenceNLL (LossFunctions.scala:76-108): sum over the time steps of the sum-reduced NLL / the number of targets
// that are not `ignore`; that number is also the example count.  total_or_null: the undivided sum (= loss * count, on the device).
// While a graph is being captured nothing has run, so the count cannot be read: the count returned then is that of ALL targets
// (time * batch); the loss and the sum are device values and are exact on every replay.
std::pair<Var, int64_t> sequence_nll(const Var& out, const Ten& target, const Ten& classWeights, int64_t ignore, Ten* total_or_null = nullptr);
// the run-time form of LAMP_RECURRENT_FUSED (its initial value)
bool recurrent_fused();
bool set_recurrent_fused(bool on);   // returns the previous value

}  // namespace F

// StatefulModule[Variable, Variable, S] (Module.scala): S flattened to `slots` Variables; an empty / all-null state = None
struct StatefulModule : Module {
  virtual int slots() const = 0;
  virtual Var forward_stateful(const Var& x, const std::vector<Var>& state, std::vector<Var>& state_out) = 0;
  Var forward(const Var& x) override { std::vector<Var> so; return forward_stateful(x, {}, so); }
  // InitState (Module.scala): empty = the reference's None; WithInit carries one
  virtual std::vector<Var> init_state() { return {}; }
};
struct Recurrent : StatefulModule {   // RNN / GRU / LSTM: the case classes' fields in `state` order
  enum Kind { kRNN = 0, kGRU = 1, kLSTM = 2 } kind;
  std::vector<Var> w;
  Recurrent(Kind k, std::vector<Var> w_);
  static Mod make(Kind k, int64_t in, int64_t hidden, int dtype, int device);   // the factories' initialisers
  void collect_state(std::vector<Var>& o) override { for (auto& v : w) o.push_back(v); }
  int slots() const override { return kind == kLSTM ? 2 : 1; }
  Var forward_stateful(const Var& x, const std::vector<Var>& state, std::vector<Var>& state_out) override;
};
struct SeqLinear : Module {
  Var weight, bias;
  SeqLinear(Var w, Var b) : weight(std::move(w)), bias(std::move(b)) {}
  static Mod make(int64_t in, int64_t out, int dtype, int device);
  void collect_state(std::vector<Var>& o) override { o.push_back(weight); o.push_back(bias); }
  Var forward(const Var& x) override { return F::seq_linear(x, weight, bias); }
};
// statefulSequence(m1, ..., mN) (StatefulSeq.scala): stateless members are lifted (state Unit, no slot)
struct StatefulSequence : StatefulModule {
  std::vector<Mod> mods;
  explicit StatefulSequence(std::vector<Mod> m) : mods(std::move(m)) {}
  void collect_state(std::vector<Var>& o) override { for (auto& m : mods) m->collect_state(o); }
  int slots() const override;
  Var forward_stateful(const Var& x, const std::vector<Var>& state, std::vector<Var>& state_out) override;
  void set_training(bool t) override { for (auto& m : mods) m->set_training(t); }
};
// the StatefulModule behind a module handle; raises for a stateless one
StatefulModule& stateful(const Mod& m, const char* what);
// FreeRunningRNN(module, timeSteps) (FreeRunningRNN.scala): greedy generation as a differentiable composition of the wrapped module's
// forward, argmax(2) detached, and the stack of the last time steps.  x [T0, B] int64 -> (outputs [timeSteps, B, V], lastState)
struct FreeRunningRNN : StatefulModule {
  Mod module;
  int64_t timeSteps;
  FreeRunningRNN(Mod m, int64_t steps);
  void collect_state(std::vector<Var>& o) override { module->collect_state(o); }
  int slots() const override { return stateful(module, "FreeRunningRNN").slots(); }
  Var forward_stateful(const Var& x, const std::vector<Var>& state, std::vector<Var>& state_out) override;
  void set_training(bool t) override { module->set_training(t); }
  std::vector<Var> init_state() override { return stateful(module, "FreeRunningRNN").init_state(); }
};
// Seq2Seq(encoder, decoder) (Seq2Seq.scala:6-28): forward(((source, dest), state0)) = decoder.forward((dest, encoder.forward((source, state0)).state))
struct Seq2Seq : StatefulModule {
  Mod encoder, decoder;
  Seq2Seq(Mod e, Mod d);
  void collect_state(std::vector<Var>& o) override { encoder->collect_state(o); decoder->collect_state(o); }
  int slots() const override { return stateful(encoder, "Seq2Seq").slots(); }
  Var forward_stateful(const Var& x, const std::vector<Var>& state, std::vector<Var>& state_out) override;   // raises: the input is a pair
  Var forward_pair(const Var& source, const Var& dest, const std::vector<Var>& state, std::vector<Var>& state_out);
  void set_training(bool t) override { encoder->set_training(t); decoder->set_training(t); }
  std::vector<Var> init_state() override { return stateful(encoder, "Seq2Seq").init_state(); }
};
// WithInit(module, init) (Seq2Seq.scala:75-114): the module with an initial state of its own
struct WithInit : StatefulModule {
  Mod module;
  std::vector<Var> init;
  WithInit(Mod m, std::vector<Var> init_);
  void collect_state(std::vector<Var>& o) override { module->collect_state(o); }
  int slots() const override { return stateful(module, "WithInit").slots(); }
  Var forward_stateful(const Var& x, const std::vector<Var>& state, std::vector<Var>& state_out) override {
    return stateful(module, "WithInit").forward_stateful(x, state, state_out);
  }
  void set_training(bool t) override { module->set_training(t); }
  std::vector<Var> init_state() override { return init; }
};

}  // namespace host
}  // namespace lamp
