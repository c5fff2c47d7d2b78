// lamp.nn.bert - see bert.h for the reference map.
#include "bert.h"

namespace lamp {
namespace host {

// ---- BertEncoder -----------------------------------------------------------------------------------------
std::shared_ptr<BertEncoder> BertEncoder::make(int64_t maxLength, int64_t vocabularySize, int64_t segmentVocabularySize, int64_t numBlocks,
                                               int64_t embeddingDim, int64_t attentionHiddenPerHeadDim, int64_t attentionNumHeads, int64_t mlpHiddenDim,
                                               double dropout, int dtype, int device, bool linearized, const Ten& positionEmbedding) {   // :485-534
  auto m = std::make_shared<BertEncoder>();
  m->tokenEmbedding = Embedding::make(vocabularySize, embeddingDim, dtype, device);
  m->segmentEmbedding = Embedding::make(segmentVocabularySize, embeddingDim, dtype, device);
  Ten pe;
  if (positionEmbedding.defined()) {
    LAMP_CHECK(positionEmbedding.ndim() == 2 && positionEmbedding.size(0) == maxLength && positionEmbedding.size(1) == embeddingDim,
               "BertEncoder: positionEmbedding must be [" << maxLength << ", " << embeddingDim << "]");
    pe = positionEmbedding.dtype() == dtype ? ops::clone(positionEmbedding) : ops::cast(positionEmbedding, dtype);
  } else {
    // the reference builds the table in SinglePrecision whatever tOpt says and type promotion does the rest; the values are the same
    pe = positional_embedding_vaswani(maxLength, embeddingDim, kF32, device);
    if (dtype != kF32) pe = ops::cast(pe, dtype);
  }
  m->positionalEmbedding = make_param(ops::view(pe, {1, maxLength, embeddingDim}));
  for (int64_t i = 0; i < numBlocks; i++)
    m->blocks.push_back(TransformerEncoderBlock::make(embeddingDim, attentionHiddenPerHeadDim, attentionNumHeads, mlpHiddenDim, embeddingDim, dropout, dtype,
                                                      device, linearized, /*gptOrder*/ false, /*causalMask*/ false));
  return m;
}
Var BertEncoder::encode(const Var& tokens, const Var& segments, const Ten& maxLength) {   // :395-406
  LAMP_CHECK(tokens->value.ndim() == 2 && tokens->shape() == segments->shape(), "BertEncoder: tokens and segments are batch x sequence (long), of one shape");
  Var a = F::bert_embedding(tokens, segments, tokenEmbedding->weights, segmentEmbedding->weights, positionalEmbedding);
  // The batch builder hands over one length per sequence ([B], lamp.data.bert's tokenMaxLength).  multiheadAttention repeats maxLength
  // (numHeads, 1) times, which turns a 1-D tensor into [numHeads, B], a shape no mask accepts; the same length for every query of the
  // sequence, [B, T], is what that repeat is written for, so a 1-D maxLength is widened here.  A 2-D one goes through as it is.
  Ten mx = maxLength;
  if (mx.defined() && mx.ndim() == 1) {
    const int64_t B = tokens->value.size(0), T = tokens->value.size(1);
    LAMP_CHECK(mx.size(0) == B, "BertEncoder: maxLength holds " << mx.size(0) << " lengths for a batch of " << B);
    const int64_t shape[2] = {B, T};
    lamp_tensor *e = nullptr, *c = nullptr;
    HCALL(lamp_expand(&e, ops::view(mx, {B, 1}).h(), shape, 2));
    const Ten expanded(e);
    HCALL(lamp_contiguous(&c, expanded.h()));
    mx = Ten(c);
  }
  for (auto& b : blocks) a = b->block(a, mx);
  return a;
}

// ---- MaskedLanguageModelModule -----------------------------------------------------------------------------
std::shared_ptr<MaskedLanguageModelModule> MaskedLanguageModelModule::make(int64_t inputDim, int64_t hiddenDim, int64_t vocabularySize, int dtype,
                                                                           int device, bool perRowPositions) {   // :347-359
  auto m = std::make_shared<MaskedLanguageModelModule>();
  m->mlp = std::make_shared<Sequential>(std::vector<Mod>{Linear::make(inputDim, hiddenDim, dtype, device, true), make_fun("relu"),
                                                         LayerNorm::make({hiddenDim}, dtype, device, false, false),
                                                         Linear::make(hiddenDim, vocabularySize, dtype, device, true)});
  m->perRowPositions = perRowPositions;
  return m;
}
Var MaskedLanguageModelModule::predict(const Var& encoderOutput, const Ten& predictionPositions) {   // :317-331
  const Ten& ev = encoderOutput->value;
  LAMP_CHECK(ev.ndim() == 3 && predictionPositions.ndim() == 2, "MaskedLanguageModelModule: encoderOutput is [B, T, D], predictionPositions [B, P] (long)");
  const int64_t B = ev.size(0), T = ev.size(1), D = ev.size(2), P = predictionPositions.size(1);
  Ten index = predictionPositions;
  if (perRowPositions) {
    LAMP_CHECK(predictionPositions.size(0) == B, "MaskedLanguageModelModule: " << predictionPositions.size(0) << " rows of positions for a batch of " << B);
    lamp_tensor* off = nullptr;
    HCALL(lamp_arange(&off, 0.0, (double)(B * T), (double)T, kI64, ev.device()));
    index = ops::add(predictionPositions, ops::view(Ten(off), {B, 1}));
  }
  Var at = F::view(F::index_select(F::view(encoderOutput, {-1, D}), 0, make_const(ops::reshape(index, {-1}))), {B, P, D});
  return mlp->forward(at);
}

// ---- BertPretrainModule --------------------------------------------------------------------------------------
std::shared_ptr<BertPretrainModule> BertPretrainModule::make(int64_t maxLength, int64_t vocabularySize, int64_t segmentVocabularySize, int64_t mlmHiddenDim,
                                                             int64_t wholeSentenceHiddenDim, int64_t numBlocks, int64_t embeddingDim,
                                                             int64_t attentionHiddenPerHeadDim, int64_t attentionNumHeads,
                                                             int64_t bertEncoderMlpHiddenDim, double dropout, int dtype, int device, bool linearized,
                                                             const Ten& positionEmbedding, bool perRowPositions) {   // :244-285
  auto m = std::make_shared<BertPretrainModule>();
  m->encoder = BertEncoder::make(maxLength, vocabularySize, segmentVocabularySize, numBlocks, embeddingDim, attentionHiddenPerHeadDim, attentionNumHeads,
                                 bertEncoderMlpHiddenDim, dropout, dtype, device, linearized, positionEmbedding);
  m->mlm = MaskedLanguageModelModule::make(embeddingDim, mlmHiddenDim, vocabularySize, dtype, device, perRowPositions);
  m->wholeSentenceBinaryClassifier = std::make_shared<Sequential>(std::vector<Mod>{
      Linear::make(embeddingDim, wholeSentenceHiddenDim, dtype, device, true), make_fun("tanh"), Linear::make(wholeSentenceHiddenDim, 1, dtype, device, true)});
  return m;
}
BertPretrainOutput BertPretrainModule::run(const Var& tokens, const Var& segments, const Ten& positions, const Ten& maxLength) {   // :216-228
  BertPretrainOutput r;
  r.encoded = encoder->encode(tokens, segments, maxLength);
  r.languageModelScores = F::log_softmax(mlm->predict(r.encoded, positions), 2);
  r.wholeSentenceBinaryClassifierScore = F::view(wholeSentenceBinaryClassifier->forward(F::select(r.encoded, 1, 0)), {-1});
  return r;
}

// ---- BertLoss ----------------------------------------------------------------------------------------------
std::shared_ptr<BertLoss> BertLoss::make(int64_t maxLength, int64_t vocabularySize, int64_t segmentVocabularySize, int64_t mlmHiddenDim,
                                         int64_t wholeSentenceHiddenDim, int64_t numBlocks, int64_t embeddingDim, int64_t attentionHiddenPerHeadDim,
                                         int64_t attentionNumHeads, int64_t bertEncoderMlpHiddenDim, double dropout, int64_t padToken, int dtype,
                                         int device, bool linearized, const Ten& positionEmbedding, bool perRowPositions) {   // :96-140
  auto m = std::make_shared<BertLoss>();
  m->pretrain = BertPretrainModule::make(maxLength, vocabularySize, segmentVocabularySize, mlmHiddenDim, wholeSentenceHiddenDim, numBlocks, embeddingDim,
                                         attentionHiddenPerHeadDim, attentionNumHeads, bertEncoderMlpHiddenDim, dropout, dtype, device, linearized,
                                         positionEmbedding, perRowPositions);
  m->classWeights = ops::ones({vocabularySize}, dtype, device);
  m->padToken = padToken;
  return m;
}
Var BertLoss::loss(const Var& tokens, const Var& segments, const Ten& positions, const Ten& maxLength, const Ten& maskedLanguageModelTarget,
                   const Ten& wholeSentenceTarget) {   // :48-62
  BertPretrainOutput o = pretrain->run(tokens, segments, positions, maxLength);
  Var l1 = F::nll_loss(F::flatten(o.languageModelScores, 0, 1), ops::reshape(maskedLanguageModelTarget, {-1}), classWeights, /*Mean*/ 1, padToken);
  Var l2 = F::binary_cross_entropy_with_logits(o.wholeSentenceBinaryClassifierScore, wholeSentenceTarget, Ten(), /*Mean*/ 1);
  return F::add(l1, l2);
}

}  // namespace host
}  // namespace lamp
