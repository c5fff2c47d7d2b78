// autoregressiveInference - see generate.h and DESIGN.md section 18.
#include "generate.h"

#include <atomic>

namespace lamp {
namespace host {

namespace {
std::atomic<bool> g_decode_fused{kDecodeFusedDefault};
std::atomic<int> g_last_path{-1};

Ten slice(const Ten& a, int64_t dim, int64_t start, int64_t end) { return ops::slice(a, dim, start, end, 1); }
Ten contiguous(const Ten& a) { lamp_tensor* o = nullptr; HCALL(lamp_contiguous(&o, a.h())); return Ten(o); }
Ten arange(int64_t start, int64_t end, int64_t step, int device) {
  lamp_tensor* o = nullptr;
  HCALL(lamp_arange(&o, (double)start, (double)end, (double)step, kI64, device));
  return Ten(o);
}
// the rows of encoded.view(-1, D) that hold the last position of every sequence of a [B, w] window, as run()'s `positions` [B, 1]
Ten last_positions(int64_t B, int64_t w, int device) { return ops::view(arange(w - 1, B * w, w, device), {B, 1}); }
Ten empty(const std::vector<int64_t>& s, int dtype, int device) {
  lamp_tensor* o = nullptr;
  HCALL(lamp_empty(&o, s.data(), (int)s.size(), dtype, device));
  return Ten(o);
}
lamp_tensor* h_or_null(const Var& v) { return v ? v->value.h() : nullptr; }

Ten decode_linear(const Ten& x, const Ten& w, bool transposed, const LayerNorm* ln, const Var& bias, int act, const Var& scale, const Ten& residual) {
  lamp_tensor* o = nullptr;
  HCALL(lamp_decode_linear(&o, x.h(), w.h(), transposed ? 1 : 0, ln ? 1 : 0, ln ? ln->eps : 0.0, ln ? h_or_null(ln->scale) : nullptr,
                           ln ? h_or_null(ln->bias) : nullptr, h_or_null(bias), act, h_or_null(scale), residual.h()));
  return Ten(o);
}

// asEval for the length of the call: the blocks' flags are put back as they were
struct EvalGuard {
  LanguageModelModule& lm;
  std::vector<bool> was;
  explicit EvalGuard(LanguageModelModule& m) : lm(m) {
    for (auto& b : lm.encoder->blocks) { was.push_back(b->train); b->train = false; }
  }
  ~EvalGuard() { for (size_t i = 0; i < was.size(); i++) lm.encoder->blocks[i]->train = was[i]; }
};

// logits [B, V] of the last position of a [B, w] window through the module's own forward
Ten window_logits(LanguageModelModule& lm, const Ten& tokens, int64_t len, int64_t w, const Ten& positions) {
  Var window = make_const(contiguous(slice(tokens, 1, len - w, len)));
  Var logits = lm.run(window, Ten(), positions).second;          // [B, 1, V]
  return ops::view(logits->value, {logits->value.size(0), -1});
}
}  // namespace

bool decode_fused() { return g_decode_fused.load(); }
bool set_decode_fused(bool on) { return g_decode_fused.exchange(on); }
int last_generate_path() { return g_last_path.load(); }

Generated language_model_generate(LanguageModelModule& lm, const Ten& prefix0, int64_t length, double temperature, int64_t M, bool wantLogits) {
  LAMP_CHECK(prefix0.defined() && prefix0.dtype() == kI64 && prefix0.ndim() == 2, "prefix must be int64 [B, P]");
  const int64_t B = prefix0.size(0), P = prefix0.size(1);
  LAMP_CHECK(B >= 1 && P >= 1, "an empty prefix: the model has nothing to continue");
  LAMP_CHECK(temperature > 0.0, "assertion failed: temperature > 0 (languagemodel/package.scala:42), got " << temperature);
  LAMP_CHECK(length >= 0, "length must not be negative, got " << length);
  const Ten& tokW = lm.tokenEmbedding->weights->value;
  const Ten& posW = lm.positionEmbedding->weights->value;
  LAMP_CHECK(M >= 1 && M <= posW.size(0), "modelBlockSize " << M << " is outside the position table of " << posW.size(0) << " rows");
  const int dev = tokW.device(), dt = tokW.dtype();
  const int64_t V = tokW.size(0), D = tokW.size(1);

  Generated g;
  g.tokens = empty({B, P + length}, kI64, dev);
  ops::copy_(slice(g.tokens, 1, 0, P), prefix0);
  if (wantLogits) g.logits = empty({B, length, V}, dt, dev);
  auto keep_logits = [&](int64_t i, const Ten& logits) {
    if (wantLogits) ops::copy_(ops::select(g.logits, 1, i), logits);
  };
  EvalGuard eval(lm);

  bool fused = decode_fused() && B <= LAMP_DECODE_MAX_ROWS && (dt == kF32 || dt == kF64 || dt == kBF16) && !MultiheadAttention::fused_call_as_written();
  // the attention's own dropout flag never leaves training mode (TrainingMode.identity, Transformer.scala:644-645): a model that has one runs the chain
  for (auto& b : lm.encoder->blocks) fused = fused && !b->attention->linearized && b->gptOrder && !(b->attention->dropout > 0.0 && b->attention->train);
  g_last_path.store(fused ? 1 : 0);
  if (length == 0) return g;

  if (!fused) {
    // the reference's loop (package.scala:88-112): the whole model over takeRight(modelBlockSize), one row of logits, multinomial
    for (int64_t i = 0; i < length; i++) {
      const int64_t len = P + i, w = std::min(len, M);
      Ten logits = window_logits(lm, g.tokens, len, w, last_positions(B, w, dev));
      keep_logits(i, logits);
      lamp_tensor* lsm = nullptr;
      HCALL(lamp_log_softmax(&lsm, ops::mul_scalar(logits, 1.0 / temperature).h(), 1));
      Ten probs = ops::exp(Ten(lsm));
      lamp_tensor* sample = nullptr;
      HCALL(lamp_multinomial(&sample, probs.h(), 1, 0));
      ops::copy_(slice(g.tokens, 1, len, len + 1), Ten(sample));
    }
    return g;
  }

  auto sample_into = [&](int64_t column, const Ten& logits) {
    HCALL(lamp_sample_logits_out(ops::select(g.tokens, 1, column).h(), logits.h(), temperature, nullptr));
  };
  const auto& blocks = lm.encoder->blocks;
  const int64_t w0 = std::min(P, M);
  const bool cached = P < M && length > 1;          // at least one token comes while the sequence still fits the context
  std::vector<Ten> wqkv, kcache, vcache;
  int64_t H = 1, d = 1;
  {
    // the first window through the operators of the training forward (TransformerEncoderBlock::block on constants), and per block the
    // key and value projections of its rows into the cache
    Var window = make_const(contiguous(slice(g.tokens, 1, P - w0, P)));
    Var pos = make_const(ops::view(arange(0, w0, 1, dev), {1, w0}));
    Var x = F::add(lm.tokenEmbedding->forward(window), lm.positionEmbedding->forward(pos));
    for (auto& b : blocks) {
      Var normed;
      x = b->block(x, Ten(), cached ? &normed : nullptr);
      if (!cached) continue;
      auto& att = *b->attention;
      H = att.numHeads;
      const int64_t HD = att.wK->value.size(1);
      LAMP_CHECK(HD % H == 0 && att.wQ->value.size(1) == HD && att.wV->value.size(1) == HD, "the attention projections differ in width");
      d = HD / H;
      wqkv.push_back(ops::cat({att.wQ->value, att.wK->value, att.wV->value}, 1));
      Ten rows = ops::view(normed->value, {B * w0, D});
      Ten kc = empty({B, H, M, d}, dt, dev), vc = empty({B, H, M, d}, dt, dev);
      // [B * w0, H d] -> [B, w0, H, d] -> [B, H, w0, d], copied into positions 0 .. w0 - 1
      ops::copy_(slice(kc, 2, 0, w0), ops::transpose(ops::view(ops::mm(rows, att.wK->value), {B, w0, H, d}), 1, 2));
      ops::copy_(slice(vc, 2, 0, w0), ops::transpose(ops::view(ops::mm(rows, att.wV->value), {B, w0, H, d}), 1, 2));
      kcache.push_back(kc); vcache.push_back(vc);
    }
    Var encoded = lm.finalNorm->forward(x);
    Ten last = ops::index_select(ops::view(encoded->value, {B * w0, D}), 0, ops::view(last_positions(B, w0, dev), {-1}));
    Ten logits = ops::mm(last, ops::transpose(tokW, 0, 1));
    keep_logits(0, logits);
    sample_into(P, logits);
  }
  Ten slidingPositions;
  for (int64_t i = 1; i < length; i++) {
    const int64_t len = P + i;        // the sequence so far; its last token sits at position t = len - 1 of the window
    Ten logits;
    if (len <= M) {
      const int64_t t = len - 1;
      lamp_tensor* e = nullptr;
      HCALL(lamp_decode_embedding(&e, tokW.h(), posW.h(), ops::select(g.tokens, 1, t).h(), t));
      Ten x(e);
      for (size_t bi = 0; bi < blocks.size(); bi++) {
        auto& b = *blocks[bi];
        Ten qkv = decode_linear(x, wqkv[bi], false, b.layerNorm1.get(), nullptr, LAMP_DECODE_ACT_NONE, nullptr, Ten());
        lamp_tensor* a = nullptr;
        HCALL(lamp_decode_attention(&a, qkv.h(), kcache[bi].h(), vcache[bi].h(), t, H));
        Ten x2 = decode_linear(Ten(a), b.attention->wO->value, false, nullptr, nullptr, LAMP_DECODE_ACT_NONE, b.scale1, x);
        Ten hid = decode_linear(x2, b.w1->value, false, b.layerNorm2.get(), b.b1, LAMP_DECODE_ACT_GELU, nullptr, Ten());
        x = decode_linear(hid, b.w2->value, false, nullptr, b.b2, LAMP_DECODE_ACT_NONE, b.scale2, x2);
      }
      logits = decode_linear(x, tokW, true, lm.finalNorm.get(), nullptr, LAMP_DECODE_ACT_NONE, nullptr, Ten());
    } else {
      // the window has slid: every cached position's embedding has moved, the cache is dead for good
      if (!slidingPositions.defined()) slidingPositions = last_positions(B, M, dev);
      logits = window_logits(lm, g.tokens, len, M, slidingPositions);
    }
    keep_logits(i, logits);
    sample_into(len, logits);
  }
  return g;
}

}  // namespace host
}  // namespace lamp
