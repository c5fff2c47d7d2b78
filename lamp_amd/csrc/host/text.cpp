// lamp.data.Text's generation - see text.h and DESIGN.md section 19.
#include "text.h"
#include "transformer.h"

#include <algorithm>
#include <atomic>

namespace lamp {
namespace host {

namespace {
std::atomic<bool> g_text_fused{kTextFusedDefault};
std::atomic<int> g_last_path{-1};

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

// Embedding -> RNN | GRU | LSTM -> [relu] -> SeqLinear -> [logSoftMax(2)], possibly inside WithInit
struct TextModel {
  StatefulModule* whole = nullptr;
  Embedding* embedding = nullptr;
  Recurrent* cell = nullptr;
  SeqLinear* linear = nullptr;
  bool relu = false, logSoftMax = false;
};
bool match(const Mod& module, TextModel& tm) {
  Module* m = module.get();
  while (auto* wi = dynamic_cast<WithInit*>(m)) m = wi->module.get();
  auto* seq = dynamic_cast<StatefulSequence*>(m);
  if (!seq) return false;
  const auto& mods = seq->mods;
  size_t at = 0;
  auto fun = [&](const char* tag) -> Fun* {
    if (at >= mods.size()) return nullptr;
    auto* f = dynamic_cast<Fun*>(mods[at].get());
    return f && f->tag == tag ? f : nullptr;
  };
  if (at >= mods.size() || !(tm.embedding = dynamic_cast<Embedding*>(mods[at].get()))) return false;
  at++;
  if (at >= mods.size() || !(tm.cell = dynamic_cast<Recurrent*>(mods[at].get()))) return false;
  at++;
  if (fun("relu")) { tm.relu = true; at++; }
  if (at >= mods.size() || !(tm.linear = dynamic_cast<SeqLinear*>(mods[at].get()))) return false;
  at++;
  if (Fun* f = fun("logsoftmax")) {
    if ((int64_t)f->a != 2) return false;
    tm.logSoftMax = true;
    at++;
  }
  if (at != mods.size()) return false;
  // one type, f32 or f64, one device
  const Ten& table = tm.embedding->weights->value;
  const int dt = table.dtype();
  if (dt != kF32 && dt != kF64) return false;
  if (!table.h()->is_device() || table.ndim() != 2) return false;
  auto with_table = [&](const Var& v) { return v->value.h()->is_device() && v->value.dtype() == dt && v->value.device() == table.device(); };
  for (auto& v : tm.cell->w) if (!with_table(v)) return false;
  if (!with_table(tm.linear->weight) || !with_table(tm.linear->bias)) return false;
  return true;
}

// the per-token state of the fused path: packed weights and two sets of state buffers that take turns
struct Stepper {
  const TextModel& tm;
  int kind, dt, dev;
  int64_t H;
  Ten w, bias, wh2;
  Ten h, c;                 // the current state [rows, H]
  Stepper(const TextModel& tm_, const std::vector<Var>& state) : tm(tm_) {
    kind = (int)tm.cell->kind;
    const Ten& table = tm.embedding->weights->value;
    dt = table.dtype(); dev = table.device();
    std::vector<lamp_tensor*> ts;
    for (auto& v : tm.cell->w) ts.push_back(v->value.h());
    lamp_tensor *wo = nullptr, *bo = nullptr, *w2 = nullptr;
    HCALL(lamp_recurrent_decode_pack(&wo, &bo, &w2, kind, ts.data(), (int)ts.size()));
    w = Ten(wo); bias = Ten(bo); wh2 = Ten(w2);
    h = dense(state.at(0)->value);
    if (kind == Recurrent::kLSTM) c = dense(state.at(1)->value);
    H = h.size(1);
  }
  // one token per row; parent: which row of the current state a row continues (undefined: its own).  Returns the module's output [rows, V]
  // written into `out` and its argmax into `tokens_out`.
  void step(const Ten& tokens, const Ten& parent, int64_t rows, const Ten& out, const Ten& tokens_out) {
    Ten hn = empty({rows, H}, dt, dev), cn, rl;
    if (kind == Recurrent::kLSTM) cn = empty({rows, H}, dt, dev);
    if (tm.relu) rl = empty({rows, H}, dt, dev);
    HCALL(lamp_recurrent_decode_step(kind, tm.embedding->weights->value.h(), tokens.h(), parent.h(), w.h(), bias.h(), wh2.h(), h.h(), c.h(), hn.h(), cn.h(),
                                     rl.h()));
    h = hn; c = cn;
    lamp_tensor* logits = nullptr;
    HCALL(lamp_decode_linear(&logits, (tm.relu ? rl : hn).h(), tm.linear->weight->value.h(), 0, 0, 0.0, nullptr, nullptr, tm.linear->bias->value.h(),
                             LAMP_DECODE_ACT_NONE, nullptr, nullptr));
    Ten lg(logits);
    HCALL(lamp_log_softmax_argmax_rows(out.h(), tokens_out.h(), lg.h(), tm.logSoftMax ? 1 : 0));
  }
};

// the module's forward over the prefix: the last time step's output [B, V] and the state
Ten prefix_forward(StatefulModule& m, const Ten& prefix, std::vector<Var>& state) {
  Var output = m.forward_stateful(make_const(prefix), m.init_state(), state);
  LAMP_CHECK(output->value.ndim() == 3, "the module's output " << output->value.h()->describe() << " must be [time, batch, dim]");
  return ops::select(output->value, 0, output->value.size(0) - 1);
}
void check_prefix(const Ten& prefix) {
  LAMP_CHECK(prefix.defined() && prefix.dtype() == kI64 && prefix.ndim() == 2 && prefix.size(0) >= 1 && prefix.size(1) >= 1,
             "the prediction batch must be int64 [time, batch] with at least one token per row");
}
}  // namespace

bool text_fused() { return g_text_fused.load(); }
bool set_text_fused(bool on) { return g_text_fused.exchange(on); }
int last_text_path() { return g_last_path.load(); }

Predicted sequence_prediction(const Mod& module, const Ten& prefix, int64_t steps) {
  StatefulModule& m = stateful(module, "sequencePrediction");
  check_prefix(prefix);
  LAMP_CHECK(steps >= 1, "steps must be positive, got " << steps);
  const int64_t B = prefix.size(1);
  TextModel tm;
  const bool fused = text_fused() && B <= LAMP_DECODE_MAX_ROWS && prefix.h()->is_device() && match(module, tm);
  g_last_path.store(fused ? 1 : 0);
  Predicted r;
  if (!fused) {                                                                      // Text.scala:27-35
    FreeRunningRNN free(module, steps);
    std::vector<Var> state;
    Var outputs = free.forward_stateful(make_const(prefix), m.init_state(), state);
    r.outputs = outputs->value;
    r.tokens = F::argmax(outputs, 2, false)->value;
    return r;
  }
  std::vector<Var> state;
  Ten first = prefix_forward(m, prefix, state);                                      // [B, V], already through the module's own tail
  const int64_t V = first.size(1);
  r.outputs = empty({steps, B, V}, first.dtype(), first.device());
  r.tokens = empty({steps, B}, kI64, first.device());
  HCALL(lamp_log_softmax_argmax_rows(ops::select(r.outputs, 0, 0).h(), ops::select(r.tokens, 0, 0).h(), first.h(), 0));
  if (steps == 1) return r;
  Stepper st(tm, state);
  for (int64_t i = 1; i < steps; i++)                                                // the token never visits the host
    st.step(ops::select(r.tokens, 0, i - 1), Ten(), B, ops::select(r.outputs, 0, i), ops::select(r.tokens, 0, i));
  return r;
}

std::vector<BeamResult> sequence_prediction_beam(const Mod& module, const Ten& prefix, int64_t steps, int64_t startSequence, int64_t endOfSequence,
                                                 int64_t k) {
  StatefulModule& m = stateful(module, "sequencePredictionBeam");
  check_prefix(prefix);
  LAMP_CHECK(prefix.size(1) == 1, "sequencePredictionBeam takes one prefix, got a batch of " << prefix.size(1));
  LAMP_CHECK(steps >= 0 && k >= 1, "steps must not be negative and k must be positive, got " << steps << " and " << k);
  TextModel tm;
  const bool fused = text_fused() && k <= LAMP_DECODE_MAX_ROWS && prefix.h()->is_device() && match(module, tm);
  g_last_path.store(fused ? 1 : 0);

  // a beam: its tokens (the first is the prefix's last), its log-probability, and where its state is - a row of the stepper's current
  // state (fused) or the Variables themselves (chain)
  struct Beam {
    std::vector<int64_t> tokens;
    double logProb = 0.0;
    int64_t lastToken = 0;
    bool atPrefix = true;          // its next input is the whole prefix
    int64_t row = 0;
    std::vector<Var> state;
  };
  std::vector<int64_t> last(1);
  {
    Ten lastTok = dense(ops::select(prefix, 0, prefix.size(0) - 1));
    HCALL(lamp_copy_to_host(lastTok.h(), last.data(), sizeof(int64_t)));
  }
  std::vector<Beam> beams(1);
  beams[0].tokens = {last[0]};
  beams[0].lastToken = startSequence;
  beams[0].state = m.init_state();
  const int dev = prefix.device();
  std::unique_ptr<Stepper> stepper;

  for (int64_t n = 0; n < steps; n++) {
    std::vector<int> live;                       // the beams that run the module this step, in order
    for (size_t b = 0; b < beams.size(); b++) if (beams[b].lastToken != endOfSequence) live.push_back((int)b);
    if (live.empty()) break;                     // every beam is carried unchanged from here on
    const int64_t rows = (int64_t)live.size();
    Ten out;                                     // the module's last-step outputs of the live beams [rows, V]
    std::vector<std::vector<Var>> nextState(rows);
    if (beams[live[0]].atPrefix) {               // the first step: one beam, the whole prefix through the module's own forward
      out = dense(prefix_forward(m, prefix, nextState[0]));
      if (fused) stepper.reset(new Stepper(tm, nextState[0]));
    } else if (fused) {
      std::vector<int64_t> tp(2 * rows);         // tokens over parents
      for (int64_t r = 0; r < rows; r++) { tp[r] = beams[live[r]].lastToken; tp[rows + r] = beams[live[r]].row; }
      Ten both = empty({2, rows}, kI64, dev);
      HCALL(lamp_copy_from_host(both.h(), tp.data(), tp.size() * sizeof(int64_t)));
      const int64_t V = tm.linear->weight->value.size(1);
      out = empty({rows, V}, stepper->dt, dev);
      Ten best = empty({rows}, kI64, dev);
      stepper->step(ops::select(both, 0, 0), ops::select(both, 0, 1), rows, out, best);
    } else {
      std::vector<Ten> outs;
      for (int64_t r = 0; r < rows; r++) {       // Text.scala:75-84, a forward per beam
        Beam& bm = beams[live[r]];
        Ten tok = empty({1, 1}, kI64, dev);
        HCALL(lamp_copy_from_host(tok.h(), &bm.lastToken, sizeof(int64_t)));
        Var output = m.forward_stateful(make_const(tok), bm.state, nextState[r]);
        outs.push_back(ops::view(output->value, {1, -1}));
      }
      out = outs.size() == 1 ? dense(outs[0]) : ops::cat(outs, 0);
    }
    // the k best entries of every live row, one read: [rows, 2 kk] doubles, values then indices
    const int64_t V = out.size(1), kk = std::min(k, V);
    lamp_tensor *tv = nullptr, *ti = nullptr;
    HCALL(lamp_topk(&tv, &ti, out.h(), kk, 1, 1, 1));
    Ten vals(tv), idx(ti);
    Ten packed = ops::cat({ops::cast(vals, kF64), ops::cast(idx, kF64)}, 1);
    std::vector<double> host(rows * 2 * kk);
    HCALL(lamp_copy_to_host(packed.h(), host.data(), host.size() * sizeof(double)));

    // candidates in the reference's order (beams in order, a finished beam as itself), sorted by sortBy(_._3).reverse: among equal sums
    // the later candidate first
    struct Cand { int beam; int64_t token; double logProb; int64_t liveRow; int64_t order; };
    std::vector<Cand> cands;
    int64_t liveAt = 0;
    for (size_t b = 0; b < beams.size(); b++) {
      if (beams[b].lastToken == endOfSequence) { cands.push_back({(int)b, -1, beams[b].logProb, -1, (int64_t)b * (V + 1)}); continue; }
      const int64_t r = liveAt++;
      for (int64_t j = 0; j < kk; j++) {
        const int64_t token = (int64_t)host[r * 2 * kk + kk + j];
        cands.push_back({(int)b, token, host[r * 2 * kk + j] + beams[b].logProb, r, (int64_t)b * (V + 1) + token});
      }
    }
    std::sort(cands.begin(), cands.end(), [](const Cand& x, const Cand& y) { return x.logProb != y.logProb ? x.logProb > y.logProb : x.order > y.order; });
    if ((int64_t)cands.size() > k) cands.resize(k);
    std::vector<Beam> next;
    for (const Cand& cd : cands) {
      Beam nb = beams[cd.beam];
      if (cd.token >= 0) {
        nb.tokens.push_back(cd.token);
        nb.logProb = cd.logProb;
        nb.lastToken = cd.token;
        nb.atPrefix = false;
        nb.row = cd.liveRow;
        nb.state = nextState[cd.liveRow];
      }
      next.push_back(std::move(nb));
    }
    beams = std::move(next);
  }
  std::stable_sort(beams.begin(), beams.end(), [](const Beam& x, const Beam& y) { return x.logProb > y.logProb; });
  std::vector<BeamResult> result;
  for (auto& b : beams) result.push_back({b.tokens, b.logProb});
  return result;
}

}  // namespace host
}  // namespace lamp
