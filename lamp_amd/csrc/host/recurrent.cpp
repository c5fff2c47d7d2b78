// lamp.nn's recurrent family - see recurrent.h for the reference map.
#include "recurrent.h"
#include "../core/switches.h"
#include <atomic>

namespace lamp {
namespace host {

namespace {
std::atomic<int> g_fused{-1};   // -1: not read yet (the switch table's value)

Ten empty(const std::vector<int64_t>& s, int dtype, int device) {
  lamp_tensor* o = nullptr;
  HCALL(lamp_empty(&o, s.data(), (int)s.size(), dtype, device));
  return Ten(o);
}
Ten dense(const Ten& t) {
  lamp_tensor* o = nullptr;
  HCALL(lamp_contiguous(&o, t.h()));
  return Ten(o);
}
Ten linear_bias(const Ten& x, const Ten& w, const Ten& b) {
  lamp_tensor* o = nullptr;
  HCALL(lamp_linear_bias(&o, x.h(), w.h(), b.h()));
  return Ten(o);
}
// out = beta * out + a . b   |   a^T . b   |   a . b^T
void gemm(const Ten& out, const Ten& a, const Ten& b, double beta) { HCALL(lamp_addmm_out(out.h(), out.h(), a.h(), b.h(), beta, 1.0)); }
void gemm_t1(const Ten& out, const Ten& a, const Ten& b, double beta) { HCALL(lamp_addmm_out_transposed1(out.h(), out.h(), a.h(), b.h(), beta, 1.0)); }
void gemm_t2(const Ten& out, const Ten& a, const Ten& b, double beta) { HCALL(lamp_addmm_out_transposed2(out.h(), out.h(), a.h(), b.h(), beta, 1.0)); }
Ten cat_columns(const std::vector<Var>& w, std::initializer_list<int> which, bool as_row) {
  std::vector<Ten> ts;
  for (int k : which) ts.push_back(as_row ? ops::reshape(w[k]->value, {1, -1}) : w[k]->value);
  return ts.size() == 1 ? dense(ts[0]) : ops::cat(ts, 1);
}

// where the gradient of one parameter lives in the packed gradients
struct Piece { int param; int packed; int64_t block; };   // packed: 0 dWx, 1 dWh (first recurrent product), 2 dWh2 (GRU's candidate), 3 bias
// What the one backward of a sequence node shares between the node's closures during one backprop.
struct SeqState {
  int kind = 0;                 // Recurrent::Kind
  int64_t T = 0, B = 0, In = 0, H = 0, nG = 0;
  // saved by forward, private to the node except `hbuf` / `cbuf`, whose rows 1 .. T are the results' values
  Ten x2, Wx, Wh, Wh2, G, hbuf, cbuf, rh;
  std::vector<Piece> pieces;
  // one backprop: the results' incoming derivatives, then what bptt() made of them
  Ten dOut, dH, dC;
  bool done = false;
  Ten dG2, dh0, dc0, dWx, dWh, dWh2, dB, dX;
  void reset() { dOut = dH = dC = Ten(); done = false; dG2 = dh0 = dc0 = dWx = dWh = dWh2 = dB = dX = Ten(); }
  void bptt();
};

void SeqState::bptt() {
  if (done) return;
  done = true;
  const int dt = G.dtype(), dev = G.device();
  Ten dG = empty({T, B, nG * H}, dt, dev);
  Ten dh = empty({B, H}, dt, dev), dc, drh;
  if (kind == Recurrent::kLSTM) dc = empty({B, H}, dt, dev);
  if (kind == Recurrent::kGRU) drh = empty({B, H}, dt, dev);
  Ten dOutC = dOut.defined() ? dense(dOut) : Ten(), dHC = dH.defined() ? dense(dH) : Ten(), dCC = dC.defined() ? dense(dC) : Ten();
  for (int64_t t = T - 1; t >= 0; t--) {
    const bool last = t == T - 1;
    Ten Gt = ops::select(G, 0, t), dGt = ops::select(dG, 0, t), hp = ops::select(hbuf, 0, t);
    Ten dOt = dOutC.defined() ? ops::select(dOutC, 0, t) : Ten();
    const lamp_tensor* dh_in = last ? dHC.h() : dh.h();
    if (kind == Recurrent::kLSTM) {
      Ten cp = ops::select(cbuf, 0, t), cn = ops::select(cbuf, 0, t + 1);
      HCALL(lamp_lstm_cell_backward(dGt.h(), dc.h(), Gt.h(), cp.h(), cn.h(), dOt.h(), dh_in, last ? dCC.h() : dc.h()));
      gemm_t2(dh, dGt, Wh, 0.0);                                     // dh_{t-1} = dG[t] . Wh^T
    } else if (kind == Recurrent::kRNN) {
      Ten hn = ops::select(hbuf, 0, t + 1);
      HCALL(lamp_rnn_cell_backward(dGt.h(), hn.h(), dOt.h(), dh_in));
      gemm_t2(dh, dGt, Wh, 0.0);
    } else {
      HCALL(lamp_gru_output_backward(dGt.h(), dh.h(), Gt.h(), hp.h(), dOt.h(), dh_in));
      gemm_t2(drh, ops::slice(dGt, 1, 2 * H, 3 * H, 1), Wh2, 0.0);   // d(r * h) = dG_h . Whh^T
      HCALL(lamp_gru_gates_backward(dGt.h(), dh.h(), Gt.h(), hp.h(), drh.h()));
      gemm_t2(dh, ops::slice(dGt, 1, 0, 2 * H, 1), Wh, 1.0);         // dh_{t-1} += dG_rz . [Whr | Whz]^T
    }
  }
  dG2 = ops::view(dG, {T * B, nG * H});
  dh0 = dh;
  dc0 = dc;
}

// packed gradients, made on demand: a constant number of launches whatever T
const Ten& packed_grad(SeqState& s, int which) {
  s.bptt();
  const int dt = s.G.dtype(), dev = s.G.device();
  if (which == 0 && !s.dWx.defined()) { s.dWx = empty({s.In, s.nG * s.H}, dt, dev); gemm_t1(s.dWx, s.x2, s.dG2, 0.0); }
  if (which == 1 && !s.dWh.defined()) {
    Ten hprev = ops::view(ops::slice(s.hbuf, 0, 0, s.T, 1), {s.T * s.B, s.H});          // all previous hidden states
    if (s.kind == Recurrent::kGRU) { s.dWh = empty({s.H, 2 * s.H}, dt, dev); gemm_t1(s.dWh, hprev, ops::slice(s.dG2, 1, 0, 2 * s.H, 1), 0.0); }
    else { s.dWh = empty({s.H, s.nG * s.H}, dt, dev); gemm_t1(s.dWh, hprev, s.dG2, 0.0); }
  }
  if (which == 2 && !s.dWh2.defined()) {
    s.dWh2 = empty({s.H, s.H}, dt, dev);
    gemm_t1(s.dWh2, ops::view(s.rh, {s.T * s.B, s.H}), ops::slice(s.dG2, 1, 2 * s.H, 3 * s.H, 1), 0.0);
  }
  if (which == 3 && !s.dB.defined()) s.dB = ops::sum_dims(s.dG2, {0}, true);
  return which == 0 ? s.dWx : which == 1 ? s.dWh : which == 2 ? s.dWh2 : s.dB;
}

bool fusable(const Var& x, const std::vector<Var>& w, const Var& h0, const Var& c0) {
  if (!F::recurrent_fused()) return false;
  const int dt = w[0]->value.dtype();
  if (dt != kF32 && dt != kF64) return false;
  auto ok = [&](const Var& v) { return !v || (v->value.h()->is_device() && v->value.dtype() == dt && v->value.device() == w[0]->value.device()); };
  if (!ok(x) || !ok(h0) || !ok(c0)) return false;
  for (auto& v : w) if (!ok(v)) return false;
  return true;
}

F::SeqResult fused(int kind, const Var& x, const std::vector<Var>& w, Var h0, Var c0) {
  LAMP_CHECK(x->value.ndim() == 3, "recurrent input " << x->value.h()->describe() << " must be [time, batch, in]");
  auto st = std::make_shared<SeqState>();
  SeqState& s = *st;
  s.kind = kind;
  s.T = x->value.size(0); s.B = x->value.size(1); s.In = x->value.size(2);
  LAMP_CHECK(s.T >= 1, "recurrent input has no time steps");
  const int dt = w[0]->value.dtype(), dev = w[0]->value.device();
  Ten bias;
  if (kind == Recurrent::kLSTM) {        // gates i | f | o | c
    s.nG = 4; s.H = w[3]->value.size(0);
    s.Wx = cat_columns(w, {0, 1, 2, 6}, false); s.Wh = cat_columns(w, {3, 4, 5, 7}, false); bias = cat_columns(w, {8, 9, 10, 11}, true);
    s.pieces = {{0, 0, 0}, {1, 0, 1}, {2, 0, 2}, {6, 0, 3}, {3, 1, 0}, {4, 1, 1}, {5, 1, 2}, {7, 1, 3}, {8, 3, 0}, {9, 3, 1}, {10, 3, 2}, {11, 3, 3}};
  } else if (kind == Recurrent::kGRU) {  // gates r | z | h
    s.nG = 3; s.H = w[1]->value.size(0);
    s.Wx = cat_columns(w, {2, 3, 0}, false); s.Wh = cat_columns(w, {4, 5}, false); s.Wh2 = dense(w[1]->value); bias = cat_columns(w, {6, 7, 8}, true);
    s.pieces = {{2, 0, 0}, {3, 0, 1}, {0, 0, 2}, {4, 1, 0}, {5, 1, 1}, {1, 2, 0}, {6, 3, 0}, {7, 3, 1}, {8, 3, 2}};
  } else {
    s.nG = 1; s.H = w[1]->value.size(0);
    s.Wx = cat_columns(w, {0}, false); s.Wh = cat_columns(w, {1}, false); bias = cat_columns(w, {2}, true);
    s.pieces = {{0, 0, 0}, {1, 1, 0}, {2, 3, 0}};
  }
  const int64_t T = s.T, B = s.B, H = s.H;
  LAMP_CHECK(s.Wx.size(0) == s.In, "recurrent input " << x->value.h()->describe() << " does not match the input weights " << s.Wx.h()->describe());
  if (!h0) h0 = make_param(ops::zeros({B, H}, dt, dev));                 // initHidden (LSTM.scala:44-52, GRU.scala:40-42, RNN.scala:27-29)
  if (kind == Recurrent::kLSTM && !c0) c0 = make_param(ops::zeros({B, H}, dt, dev));
  LAMP_CHECK(h0->shape() == (std::vector<int64_t>{B, H}), "initial hidden state " << h0->value.h()->describe() << " must be [" << B << ", " << H << "]");
  s.x2 = ops::reshape(dense(x->value), {T * B, s.In});
  s.G = ops::view(linear_bias(s.x2, s.Wx, bias), {T, B, s.nG * H});      // x.Wx + bias of every time step: one product
  s.hbuf = empty({T + 1, B, H}, dt, dev);                                // h_0 in row 0: out = rows 1 .. T, the previous states = rows 0 .. T-1
  ops::copy_(ops::select(s.hbuf, 0, 0), h0->value);
  if (kind == Recurrent::kLSTM) {
    LAMP_CHECK(c0->shape() == h0->shape(), "initial memory " << c0->value.h()->describe() << " must have the hidden state's shape");
    s.cbuf = empty({T + 1, B, H}, dt, dev);
    ops::copy_(ops::select(s.cbuf, 0, 0), c0->value);
  }
  if (kind == Recurrent::kGRU) s.rh = empty({T, B, H}, dt, dev);
  for (int64_t t = 0; t < T; t++) {
    Ten Gt = ops::select(s.G, 0, t), hp = ops::select(s.hbuf, 0, t), hn = ops::select(s.hbuf, 0, t + 1);
    if (kind == Recurrent::kLSTM) {
      gemm(Gt, hp, s.Wh, 1.0);
      HCALL(lamp_lstm_cell_forward(Gt.h(), ops::select(s.cbuf, 0, t).h(), hn.h(), ops::select(s.cbuf, 0, t + 1).h()));
    } else if (kind == Recurrent::kRNN) {
      gemm(Gt, hp, s.Wh, 1.0);
      HCALL(lamp_rnn_cell_forward(Gt.h(), hn.h()));
    } else {
      Ten rht = ops::select(s.rh, 0, t);
      gemm(ops::slice(Gt, 1, 0, 2 * H, 1), hp, s.Wh, 1.0);
      HCALL(lamp_gru_gates_forward(Gt.h(), hp.h(), rht.h()));
      gemm(ops::slice(Gt, 1, 2 * H, 3 * H, 1), rht, s.Wh2, 1.0);
      HCALL(lamp_gru_output_forward(Gt.h(), hp.h(), hn.h()));
    }
  }

  // One node holds the inputs and the backward; the results are its consumers, so the topological order runs it once, after every
  // result that has a consumer of its own has handed its derivative over (cf. convolution_pair's shared state in ops.cpp).
  auto core = std::make_shared<Op>();
  core->name = kind == Recurrent::kLSTM ? "LSTMSequence" : kind == Recurrent::kGRU ? "GRUSequence" : "RNNSequence";
  core->reset = [st]() { st->reset(); };
  core->params.push_back({x, [st](const Ten&, Variable& out) {
    SeqState& s = *st;
    s.bptt();
    Ten dx = empty({s.T * s.B, s.In}, s.G.dtype(), s.G.device());
    gemm_t2(dx, s.dG2, s.Wx, 0.0);                                        // dx = dG . Wx^T
    out.accumulate(ops::reshape(dx, out.shape()), true);
  }});
  for (const Piece& pc : s.pieces) {
    core->params.push_back({w[pc.param], [st, pc](const Ten&, Variable& out) {
      SeqState& s = *st;
      const Ten& g = packed_grad(s, pc.packed);
      Ten part = g.size(1) == s.H ? g : dense(ops::slice(g, 1, pc.block * s.H, (pc.block + 1) * s.H, 1));
      out.accumulate(ops::reshape(part, out.shape()), true);
    }});
  }
  core->params.push_back({h0, [st](const Ten&, Variable& out) { st->bptt(); out.accumulate(st->dh0, false); }});
  if (kind == Recurrent::kLSTM) core->params.push_back({c0, [st](const Ten&, Variable& out) { st->bptt(); out.accumulate(st->dc0, false); }});
  // the hub's value is a one-element marker: a result's closure installs it as the hub's gradient (same shape) to say "reached"
  Ten mark = ops::zeros({1}, dt, dev);
  Var hub = make_result(core, mark);

  auto result = [&](const char* name, const Ten& value, Ten SeqState::*slot) {
    auto op = std::make_shared<Op>();
    op->name = name;
    op->params.push_back({hub, [st, slot, mark](const Ten& p, Variable& out) {
      (*st).*slot = p;
      if (!out.has_grad()) { out.grad = mark; out.grad_shared = true; }   // the hub's closures read the slots, not this
    }});
    return make_result(op, value);
  };
  F::SeqResult r;
  r.out = result("SequenceOutput", ops::slice(s.hbuf, 0, 1, T + 1, 1), &SeqState::dOut);
  r.h = result("SequenceLastHidden", ops::select(s.hbuf, 0, T), &SeqState::dH);
  if (kind == Recurrent::kLSTM) r.c = result("SequenceLastMemory", ops::select(s.cbuf, 0, T), &SeqState::dC);
  return r;
}

// xt.mm(wx) + h.mm(wh) + b
Var gate(const Var& xt, const Var& wx, const Var& h, const Var& wh, const Var& b) { return F::add(F::add(F::mm(xt, wx), F::mm(h, wh)), b); }
Var init_hidden(const Var& x, const Var& wh) { return make_param(ops::zeros({x->value.size(1), wh->value.size(0)}, wh->value.dtype(), wh->value.device())); }
}  // namespace

namespace F {

bool recurrent_fused() {
  int v = g_fused.load();
  if (v < 0) { v = sw().recurrent_fused ? 1 : 0; g_fused.store(v); }
  return v != 0;
}
bool set_recurrent_fused(bool on) {
  const bool prev = recurrent_fused();
  g_fused.store(on ? 1 : 0);
  return prev;
}

SeqResult lstm(const Var& x, const std::vector<Var>& w, const Var& h0_, const Var& c0_) {
  LAMP_CHECK(w.size() == 12, "LSTM takes 12 state tensors (LSTM.scala:28-42)");
  LAMP_CHECK((bool)h0_ == (bool)c0_, "LSTM's state is Option[(h, c)]: both or none");
  if (fusable(x, w, h0_, c0_)) return fused(Recurrent::kLSTM, x, w, h0_, c0_);
  Var h = h0_ ? h0_ : init_hidden(x, w[4]), c = c0_ ? c0_ : init_hidden(x, w[4]);     // LSTM.scala:44-52
  std::vector<Var> outputs;
  for (int64_t t = 0; t < x->value.size(0); t++) {                                   // LSTM.scala:65-78
    Var xt = F::select(x, 0, t);
    Var it = F::sigmoid(gate(xt, w[0], h, w[3], w[8]));
    Var ft = F::sigmoid(gate(xt, w[1], h, w[4], w[9]));
    Var ot = F::sigmoid(gate(xt, w[2], h, w[5], w[10]));
    Var ccap = F::tanh(gate(xt, w[6], h, w[7], w[11]));
    Var ct = F::add(F::mult(ft, c), F::mult(it, ccap));
    Var ht = F::mult(ot, F::tanh(ct));
    outputs.push_back(ht);
    h = ht; c = ct;
  }
  return {F::stack(outputs, 0), h, c};
}
SeqResult gru(const Var& x, const std::vector<Var>& w, const Var& h0_) {
  LAMP_CHECK(w.size() == 9, "GRU takes 9 state tensors (GRU.scala:27-38)");
  if (fusable(x, w, h0_, nullptr)) return fused(Recurrent::kGRU, x, w, h0_, nullptr);
  Var h = h0_ ? h0_ : init_hidden(x, w[1]);
  std::vector<Var> outputs;
  for (int64_t t = 0; t < x->value.size(0); t++) {                                   // GRU.scala:50-60
    Var xt = F::select(x, 0, t);
    Var r = F::sigmoid(gate(xt, w[2], h, w[4], w[6]));
    Var z = F::sigmoid(gate(xt, w[3], h, w[5], w[7]));
    Var hcap = F::tanh(gate(xt, w[0], F::mult(r, h), w[1], w[8]));
    Var nh = F::add(F::mult(z, h), F::mult(F::const_add(F::const_mult(z, -1.0), 1.0), hcap));
    outputs.push_back(nh);
    h = nh;
  }
  return {F::stack(outputs, 0), h, nullptr};
}
SeqResult rnn(const Var& x, const std::vector<Var>& w, const Var& h0_) {
  LAMP_CHECK(w.size() == 3, "RNN takes 3 state tensors (RNN.scala:20-25)");
  if (fusable(x, w, h0_, nullptr)) return fused(Recurrent::kRNN, x, w, h0_, nullptr);
  Var h = h0_ ? h0_ : init_hidden(x, w[1]);
  std::vector<Var> outputs;
  for (int64_t t = 0; t < x->value.size(0); t++) {                                   // RNN.scala:38-44
    Var nh = F::tanh(gate(F::select(x, 0, t), w[0], h, w[1], w[2]));
    outputs.push_back(nh);
    h = nh;
  }
  return {F::stack(outputs, 0), h, nullptr};
}
Var seq_linear(const Var& x, const Var& weight, const Var& bias) {
  const int dt = weight->value.dtype();
  auto with_weight = [&](const Var& v) { return v->value.h()->is_device() && v->value.dtype() == dt && v->value.device() == weight->value.device(); };
  if (recurrent_fused() && x->value.ndim() == 3 && (dt == kF32 || dt == kF64) && with_weight(weight) && with_weight(x) && with_weight(bias)) {
    const int64_t T = x->value.size(0), B = x->value.size(1);                        // one product over the [T * B, in] view
    Var b2 = bias->value.ndim() == 2 ? bias : F::view(bias, {1, -1});
    return F::view(F::linear_bias(F::reshape(x, {T * B, x->value.size(2)}), weight, b2), {T, B, -1});
  }
  std::vector<Var> outputs;
  for (int64_t t = 0; t < x->value.size(0); t++) outputs.push_back(F::add(F::mm(F::select(x, 0, t), weight), bias));   // SeqLinear.scala:24-27
  return F::stack(outputs, 0);
}

std::pair<Var, int64_t> sequence_nll(const Var& out, const Ten& target, const Ten& classWeights, int64_t ignore, Ten* total_or_null) {
  LAMP_CHECK(out->value.ndim() == 3 && target.ndim() == 2, "SequenceNLL: output [time, batch, classes] and target [time, batch]");
  const int64_t T = out->value.size(0), B = out->value.size(1);
  // the reference adds T sum-reduced losses and reads T ignored counts; one loss over the [T * B, classes] view, one count, one read
  Var total = F::nll_loss(F::reshape(out, {T * B, out->value.size(2)}), ops::reshape(target, {T * B}), classWeights, 2, ignore);
  lamp_tensor* ne = nullptr;
  HCALL(lamp_ne_scalar(&ne, target.h(), (double)ignore));
  Ten kept = ops::sum_all(ops::cast(Ten(ne), kI64));   // (a sum in the mask's own type wraps at 256)
  // the division stays on the device, so the loss never waits for the host; the example count is the one host read - and none at all
  // while a graph is being captured (nothing has run yet): the count reported then is that of all targets
  Var loss = F::div(total, make_const(ops::cast(kept, out->value.dtype())));
  if (total_or_null) *total_or_null = total->value;
  int capturing = 0;
  HCALL(lamp_graph_is_capturing(&capturing));
  double n = (double)(T * B);
  if (!capturing) HCALL(lamp_item(kept.h(), &n));
  return {loss, (int64_t)n};
}

}  // namespace F

// ---- modules ---------------------------------------------------------------------------------------------------------------
Recurrent::Recurrent(Kind k, std::vector<Var> w_) : kind(k), w(std::move(w_)) {
  LAMP_CHECK(w.size() == (k == kLSTM ? 12u : k == kGRU ? 9u : 3u), "wrong number of state tensors for a recurrent module");
}
Mod Recurrent::make(Kind k, int64_t in, int64_t hidden, int dtype, int device) {
  auto X = [&]() { return make_param(ops::normal(0.0, std::sqrt(2.0 / (double)(in + hidden)), {in, hidden}, dtype, device)); };
  auto Hh = [&]() { return make_param(ops::normal(0.0, std::sqrt(2.0 / (double)(hidden + hidden)), {hidden, hidden}, dtype, device)); };
  auto b = [&]() { return make_param(ops::zeros({1, hidden}, dtype, device)); };
  std::vector<Var> w;
  if (k == kLSTM) w = {X(), X(), X(), Hh(), Hh(), Hh(), X(), Hh(), b(), b(), b(), b()};
  else if (k == kGRU) w = {X(), Hh(), X(), X(), Hh(), Hh(), b(), b(), b()};
  else w = {X(), Hh(), b()};
  return std::make_shared<Recurrent>(k, w);
}
Var Recurrent::forward_stateful(const Var& x, const std::vector<Var>& state, std::vector<Var>& state_out) {
  Var h0 = state.size() > 0 ? state[0] : nullptr, c0 = state.size() > 1 ? state[1] : nullptr;
  F::SeqResult r = kind == kLSTM ? F::lstm(x, w, h0, c0) : kind == kGRU ? F::gru(x, w, h0) : F::rnn(x, w, h0);
  state_out.push_back(r.h);
  if (kind == kLSTM) state_out.push_back(r.c);
  return r.out;
}
Mod SeqLinear::make(int64_t in, int64_t out, int dtype, int device) {
  return std::make_shared<SeqLinear>(make_param(ops::normal(0.0, std::sqrt(2.0 / (double)(in + out)), {in, out}, dtype, device)),
                                     make_param(ops::zeros({1, out}, dtype, device)));
}
int StatefulSequence::slots() const {
  int n = 0;
  for (auto& m : mods) if (auto* s = dynamic_cast<StatefulModule*>(m.get())) n += s->slots();
  return n;
}
Var StatefulSequence::forward_stateful(const Var& x, const std::vector<Var>& state, std::vector<Var>& state_out) {
  LAMP_CHECK(state.empty() || (int)state.size() == slots(), "statefulSequence: " << state.size() << " state Variables for " << slots() << " slots");
  Var v = x;
  size_t at = 0;
  for (auto& m : mods) {
    auto* s = dynamic_cast<StatefulModule*>(m.get());
    if (!s) { v = m->forward(v); continue; }                               // a lifted stateless module
    std::vector<Var> mine;
    if (!state.empty()) mine.assign(state.begin() + at, state.begin() + at + s->slots());
    bool none = true;
    for (auto& e : mine) if (e) none = false;
    if (none) mine.clear();
    at += s->slots();
    v = s->forward_stateful(v, mine, state_out);
  }
  return v;
}

// ---- FreeRunningRNN, Seq2Seq, WithInit: compositions of the modules above ------------------------------------------------------
StatefulModule& stateful(const Mod& m, const char* what) {
  auto* s = dynamic_cast<StatefulModule*>(m.get());
  LAMP_CHECK(s, what << ": not a stateful module");
  return *s;
}
FreeRunningRNN::FreeRunningRNN(Mod m, int64_t steps) : module(std::move(m)), timeSteps(steps) {
  stateful(module, "FreeRunningRNN");
  LAMP_CHECK(timeSteps >= 1, "FreeRunningRNN: timeSteps must be positive, got " << timeSteps);
}
Var FreeRunningRNN::forward_stateful(const Var& x, const std::vector<Var>& state, std::vector<Var>& state_out) {
  StatefulModule& m = stateful(module, "FreeRunningRNN");
  LAMP_CHECK(x->value.ndim() == 2, "FreeRunningRNN: input " << x->value.h()->describe() << " must be [time, batch] token ids");
  const int64_t batch = x->value.size(1);
  Var lastOutput = x;
  std::vector<Var> lastState = state, buffer;
  for (int64_t n = 0; n < timeSteps; n++) {                                  // FreeRunningRNN.scala:26-55
    std::vector<Var> next;
    Var output = m.forward_stateful(lastOutput, lastState, next);
    LAMP_CHECK(output->value.ndim() == 3, "FreeRunningRNN: the module's output " << output->value.h()->describe() << " must be [time, batch, dim]");
    const int64_t T = output->value.size(0);
    Var lastChar = T > 1 ? F::view(F::select(output, 0, T - 1), {1, output->value.size(1), output->value.size(2)}) : output;
    lastOutput = make_const(F::argmax(lastChar, 2, false)->value);           // .detached
    lastState = next;
    buffer.push_back(lastChar);
  }
  for (auto& v : lastState) state_out.push_back(v);
  return F::view(F::stack(buffer, 0), {timeSteps, batch, -1});
}
Seq2Seq::Seq2Seq(Mod e, Mod d) : encoder(std::move(e)), decoder(std::move(d)) {
  LAMP_CHECK(stateful(encoder, "Seq2Seq").slots() == stateful(decoder, "Seq2Seq").slots(),
             "Seq2Seq: the encoder's state (" << stateful(encoder, "Seq2Seq").slots() << " Variables) is the decoder's initial state ("
                                              << stateful(decoder, "Seq2Seq").slots() << ")");
}
Var Seq2Seq::forward_stateful(const Var&, const std::vector<Var>&, std::vector<Var>&) {
  LAMP_CHECK(false, "Seq2Seq takes (source, dest): call lamp_module_forward_stateful_pair");
  return nullptr;
}
Var Seq2Seq::forward_pair(const Var& source, const Var& dest, const std::vector<Var>& state, std::vector<Var>& state_out) {
  std::vector<Var> encoderState;
  stateful(encoder, "Seq2Seq").forward_stateful(source, state, encoderState);
  return stateful(decoder, "Seq2Seq").forward_stateful(dest, encoderState, state_out);
}
WithInit::WithInit(Mod m, std::vector<Var> init_) : module(std::move(m)), init(std::move(init_)) {
  LAMP_CHECK((int)init.size() == stateful(module, "WithInit").slots(),
             "WithInit: " << init.size() << " initial state Variables for " << stateful(module, "WithInit").slots() << " slots");
}

}  // namespace host
}  // namespace lamp
