// lamp.nn.bert over the C ABI: BertEncoder, MaskedLanguageModelModule, BertPretrainModule, BertLoss.
//
// Reference: lamp-core/src/main/scala/lamp/nn/bert/bert.scala (BertLoss :42-156, BertPretrainModule :209-303, MaskedLanguageModelModule
// :312-376, BertEncoder :385-535).  Tuple / case-class inputs arrive through Module::forward_multi(vars, aux tensors) as in transformer.h.
// The encoder's input embedding is F::bert_embedding (one node over the kernels of kernels/bert.hip, or the reference's chain: the
// switch is F::set_bert_fused); everything else is a composition of the operators in ops.h.
#pragma once
#include "transformer.h"

namespace lamp {
namespace host {

struct BertEncoder : Module {               // bert.scala:385-407; state: tokenEmbedding, segmentEmbedding, positionalEmbedding, blocks
  std::shared_ptr<Embedding> tokenEmbedding, segmentEmbedding;
  Var positionalEmbedding;                  // a parameter, [1, maxLength, embeddingDim]
  std::vector<std::shared_ptr<TransformerEncoderBlock>> blocks;
  // positionEmbedding undefined: PositionalEmbedding.vaswani in single precision, cast to dtype (bert.scala:510-519)
  static std::shared_ptr<BertEncoder> make(int64_t maxLength, int64_t vocabularySize, int64_t segmentVocabularySize, int64_t numBlocks,
                                           int64_t embeddingDim, int64_t attentionHiddenPerHeadDim, int64_t attentionNumHeads, int64_t mlpHiddenDim,
                                           double dropout, int dtype, int device, bool linearized, const Ten& positionEmbedding);
  void collect_state(std::vector<Var>& o) override {
    tokenEmbedding->collect_state(o); segmentEmbedding->collect_state(o); o.push_back(positionalEmbedding);
    for (auto& b : blocks) b->collect_state(o);
  }
  Var encode(const Var& tokens, const Var& segments, const Ten& maxLength);
  Var forward(const Var&) override { LAMP_CHECK(false, "BertEncoder takes (tokens, segments, maxLength?)"); return nullptr; }
  // vars = (tokens, segments); aux = (maxLength?)
  Var forward_multi(const std::vector<Var>& xs, const std::vector<Ten>& aux) override {
    LAMP_CHECK(xs.size() == 2, "BertEncoder takes (tokens, segments, maxLength?)");
    return encode(xs[0], xs[1], aux.empty() ? Ten() : aux[0]);
  }
  void set_training(bool t) override { for (auto& b : blocks) b->set_training(t); }
};

struct MaskedLanguageModelModule : Module {   // bert.scala:312-359: Linear -> relu -> LayerNorm -> Linear at the prediction positions
  std::shared_ptr<Sequential> mlp;
  // false (the reference as written): positions index the rows of encoded.view(-1, D) directly, so every batch row reads batch row 0's
  // region; true: row b's positions are offset by b * T, the intended per-row gather.  Not in the reference.
  bool perRowPositions = false;
  static std::shared_ptr<MaskedLanguageModelModule> make(int64_t inputDim, int64_t hiddenDim, int64_t vocabularySize, int dtype, int device,
                                                         bool perRowPositions);
  void collect_state(std::vector<Var>& o) override { mlp->collect_state(o); }
  Var predict(const Var& encoderOutput, const Ten& predictionPositions);
  Var forward(const Var&) override { LAMP_CHECK(false, "MaskedLanguageModelModule takes (encoderOutput, predictionPositions)"); return nullptr; }
  // vars = (encoderOutput); aux = (predictionPositions)
  Var forward_multi(const std::vector<Var>& xs, const std::vector<Ten>& aux) override {
    LAMP_CHECK(xs.size() == 1 && !aux.empty() && aux[0].defined(), "MaskedLanguageModelModule takes (encoderOutput, predictionPositions)");
    return predict(xs[0], aux[0]);
  }
  void set_training(bool t) override { mlp->set_training(t); }
};

struct BertPretrainOutput { Var encoded, languageModelScores, wholeSentenceBinaryClassifierScore; };   // bert.scala:203-207

struct BertPretrainModule : Module {        // bert.scala:209-303; state: encoder, mlm, wholeSentenceBinaryClassifier
  std::shared_ptr<BertEncoder> encoder;
  std::shared_ptr<MaskedLanguageModelModule> mlm;
  std::shared_ptr<Sequential> wholeSentenceBinaryClassifier;   // Linear -> tanh -> Linear(., 1)
  static std::shared_ptr<BertPretrainModule> make(int64_t maxLength, int64_t vocabularySize, int64_t segmentVocabularySize, int64_t mlmHiddenDim,
                                                  int64_t wholeSentenceHiddenDim, int64_t numBlocks, int64_t embeddingDim,
                                                  int64_t attentionHiddenPerHeadDim, int64_t attentionNumHeads, int64_t bertEncoderMlpHiddenDim,
                                                  double dropout, int dtype, int device, bool linearized, const Ten& positionEmbedding,
                                                  bool perRowPositions);
  void collect_state(std::vector<Var>& o) override { encoder->collect_state(o); mlm->collect_state(o); wholeSentenceBinaryClassifier->collect_state(o); }
  BertPretrainOutput run(const Var& tokens, const Var& segments, const Ten& positions, const Ten& maxLength);
  Var forward(const Var&) override { LAMP_CHECK(false, "BertPretrainModule takes BertPretrainInput: (tokens, segments), (positions, maxLength?)"); return nullptr; }
  // vars = (tokens, segments); aux = (positions, maxLength?); returns the language model scores
  Var forward_multi(const std::vector<Var>& xs, const std::vector<Ten>& aux) override {
    LAMP_CHECK(xs.size() == 2 && !aux.empty() && aux[0].defined(), "BertPretrainModule takes BertPretrainInput: (tokens, segments), (positions, maxLength?)");
    return run(xs[0], xs[1], aux[0], aux.size() > 1 ? aux[1] : Ten()).languageModelScores;
  }
  // the reference's asEval / asTraining reach the encoder and the mlm (bert.scala:287-299); the classifier has no mode
  void set_training(bool t) override { encoder->set_training(t); mlm->set_training(t); }
};

struct BertLoss : Module {                  // bert.scala:42-156: NLL(mean, ignore = padToken, class weights of ones) + BCEWithLogits(mean)
  std::shared_ptr<BertPretrainModule> pretrain;
  Ten classWeights; int64_t padToken = -100;
  static std::shared_ptr<BertLoss> make(int64_t maxLength, int64_t vocabularySize, int64_t segmentVocabularySize, int64_t mlmHiddenDim,
                                        int64_t wholeSentenceHiddenDim, int64_t numBlocks, int64_t embeddingDim, int64_t attentionHiddenPerHeadDim,
                                        int64_t attentionNumHeads, int64_t bertEncoderMlpHiddenDim, double dropout, int64_t padToken, int dtype,
                                        int device, bool linearized, const Ten& positionEmbedding, bool perRowPositions);
  void collect_state(std::vector<Var>& o) override { pretrain->collect_state(o); }
  Var loss(const Var& tokens, const Var& segments, const Ten& positions, const Ten& maxLength, const Ten& maskedLanguageModelTarget,
           const Ten& wholeSentenceTarget);
  Var forward(const Var&) override { LAMP_CHECK(false, "BertLoss takes BertLossInput: (tokens, segments), (positions, maxLength?, maskedLanguageModelTarget, wholeSentenceTarget)"); return nullptr; }
  // vars = (tokens, segments); aux = (positions, maxLength?, maskedLanguageModelTarget, wholeSentenceTarget)
  Var forward_multi(const std::vector<Var>& xs, const std::vector<Ten>& aux) override {
    LAMP_CHECK(xs.size() == 2 && aux.size() == 4 && aux[0].defined() && aux[2].defined() && aux[3].defined(),
               "BertLoss takes BertLossInput: (tokens, segments), (positions, maxLength?, maskedLanguageModelTarget, wholeSentenceTarget)");
    return loss(xs[0], xs[1], aux[0], aux[1], aux[2], aux[3]);
  }
  void set_training(bool t) override { pretrain->set_training(t); }
};

}  // namespace host
}  // namespace lamp
