/*
 * lamp_host.h - C ABI of the host-side mirror of lamp-core's autograd / nn / optimiser layer.
 *
 * In the reference this layer is Scala running on the JVM ABOVE the JNI boundary
 * (lamp-core/src/main/scala/lamp/autograd/{autograd,ops}.scala, lamp/nn (all files),
 * lamp-data/.../distributed/package.scala); it only sequences aten.* calls.  No JVM exists in
 * the build environment, so the same sequencing logic is restated in C++ over lamp_hip.h and
 * exported here so that the parity tests and bench.py can drive the exact op sequences the
 * reference would issue.  A JVM deployment does not need this header: lamp-core itself runs
 * unchanged on top of lamp_hip.h.
 *
 * Same conventions as lamp_hip.h: int status, lamp_last_error(), out-params own +1 handle.
 */
#ifndef LAMP_HOST_H
#define LAMP_HOST_H

#include "lamp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lamp_var lamp_var;             /* lamp.autograd.Variable (autograd.scala:176) */
typedef struct lamp_module lamp_module;       /* lamp.nn.GenericModule (Module.scala:272) */
typedef struct lamp_optimizer lamp_optimizer; /* lamp.nn.Optimizer (Optimizer.scala:5) */
typedef struct lamp_model lamp_model;         /* lamp.nn.SupervisedModel (SupervisedModel.scala:151) */

/* ---- variables (autograd/package.scala:60-78; autograd.scala:176-282) ---- */
int lamp_var_const(lamp_var** out, const lamp_tensor* value);
int lamp_var_param(lamp_var** out, const lamp_tensor* value);
int lamp_var_value(const lamp_var* v, lamp_tensor** out);
int lamp_var_grad(const lamp_var* v, lamp_tensor** out);          /* *out = NULL when needsGrad is false */
int lamp_var_needs_grad(const lamp_var* v, int* out);
int lamp_var_zero_grad(lamp_var* v);
int lamp_var_backprop(lamp_var* v);                               /* Variable.backprop */
int lamp_var_wengert_size(const lamp_var* v, int64_t* out);       /* length of the topological order */
int lamp_var_release(lamp_var* v);

/* One entry point for every Op case class of ops.scala, selected by its Scala name
 * ("MatMul", "Add", "Relu", "Convolution", "BatchNorm2D", "NllLoss", ...):
 *   vars    - Variable inputs in the order of the case class parameters (NULL for absent options)
 *   tensors - plain tensor arguments (targets, weights, running statistics)
 *   d / i   - double / long scalar arguments in declaration order */
int lamp_op_apply(lamp_var** out, const char* name, lamp_var* const* vars, int nvars, lamp_tensor* const* tensors, int ntensors,
                  const double* d, int nd, const int64_t* i, int ni);

/* ---- modules (lamp/nn) ---- */
int lamp_module_linear(lamp_module** out, int64_t in, int64_t outf, int dtype, int device, int bias);
int lamp_module_conv2d(lamp_module** out, int64_t in_channels, int64_t out_channels, int64_t kernel, int dtype, int device, int bias,
                       int64_t stride, int64_t padding, int64_t dilation, int64_t groups);
/* Conv1D (nn/Conv1D.scala): input [N, in, L], weights [out, in / groups, kernel] ~ N(0, sqrt(2 / (out + in))), bias zeros [out] (a
 * parameter with bias != 0, else a constant that is still part of the state).  The reference writes the weight as [out, in, kernel]
 * whatever groups is; this follows lamp_module_conv2d.
 * Conv2DTransposed (nn/Conv2DTransposed.scala): input [N, in, H, W], weights [in, out, kernel, kernel], same init, groups 1, output
 * padding 0, output (H - 1) stride - 2 padding + dilation (kernel - 1) + 1.  The reference's default is bias = false.
 * WeightNormLinear (nn/WeightNormLinear.scala): state [V [out, in] ~ N(0, sqrt(2 / (in + out))), G [1, in] ~ N(0, 0.01), bias zeros
 * [1, out] if bias]; forward x.mm(WeightNorm(V, G, dim 0).t) + bias, a composition of existing nodes.
 * bf16 / f32 convolutions of the first two run on the matrix cores (kernels/conv_gen.hip), see lamp_convolution_matrix_path. */
int lamp_module_conv1d(lamp_module** out, int64_t in_channels, int64_t out_channels, int64_t kernel, int dtype, int device, int bias,
                       int64_t stride, int64_t padding, int64_t dilation, int64_t groups);
int lamp_module_conv2d_transposed(lamp_module** out, int64_t in_channels, int64_t out_channels, int64_t kernel, int dtype, int device, int bias,
                                  int64_t stride, int64_t padding, int64_t dilation);
int lamp_module_weight_norm_linear(lamp_module** out, int64_t in, int64_t outf, int dtype, int device, int bias);
/* 1 (the default): 1-D and transposed convolutions in bf16 / f32 with groups == 1 that no specialised kernel takes run the general
 * implicit-GEMM kernels on the matrix cores (forward, input gradient, weight gradient; deterministic).  0: they run the direct kernels,
 * as f64 and grouped ones always do.  Process-wide; returns the previous value in *previous_or_null. */
int lamp_convolution_matrix_path(int on, int* previous_or_null);
int lamp_module_batch_norm(lamp_module** out, int64_t features, int dtype, int device, int two_d);
int lamp_module_layer_norm(lamp_module** out, const int64_t* shape, int nshape, int dtype, int device, int scale, int bias);
int lamp_module_dropout(lamp_module** out, double p);
int lamp_module_fun(lamp_module** out, const char* name, double a, double b);
int lamp_module_sequential(lamp_module** out, lamp_module* const* mods, int n);
int lamp_module_residual(lamp_module** out, lamp_module* right, lamp_module* left_or_null);
int lamp_module_mlp(lamp_module** out, int64_t in, int64_t outf, const int64_t* hidden, int nhidden, int dtype, int device, double dropout,
                    int last_non_linearity, const char* activation, int norm, int bias);
/* Cnn.resnet (example-cifar100/src/main/scala/lamp/example/cifar/cnn.scala:89-137) */
int lamp_module_resnet(lamp_module** out, int64_t num_classes, double dropout, int dtype, int device);
/* ---- transformer family and the autoregressive language model (lamp-core nn/Transformer.scala, nn/Embedding.scala,
 * nn/languagemodel/lm.scala).  State order = the reference's `state`; the layer norms inside the blocks carry no scale / bias
 * (LayerNorm.apply defaults).  Modules whose input is a tuple / case class are called through lamp_module_forward_multi. */
int lamp_module_embedding(lamp_module** out, int64_t classes, int64_t dimensions, int dtype, int device);            /* Embedding.scala:35-48 */
int lamp_module_multihead_attention(lamp_module** out, int64_t dQ, int64_t dK, int64_t dV, int64_t hidden_per_head, int64_t outf, double dropout,
                                    int64_t num_heads, int dtype, int device, int linearized, int causal_mask);      /* Transformer.scala:619-641; vars (q, k, v), tensors (maxLength?) */
/* What the fused-operator branch of MultiheadAttention.multiheadAttention (Transformer.scala:946-962) computes.  0 (default): the
 * arithmetic of the reference's ATen CPU path (its composed branch, :963-1001): per-head attention over the sequence; the flash
 * kernels read (batch, heads, sequence, d) views of the projections in place.  1: the call as written for CUDA - (batch, sequence,
 * heads, d) views handed to an operator that reads dimension 1 as heads (attention over the heads of each token).  Process-wide;
 * returns the previous value in *previous_or_null.  Environment default: LAMP_ATTENTION_AS_WRITTEN_FOR_CUDA=1. */
int lamp_attention_fused_call_as_written(int on, int* previous_or_null);
int lamp_module_transformer_encoder_block(lamp_module** out, int64_t in, int64_t attention_hidden_per_head, int64_t attention_num_heads,
                                          int64_t mlp_hidden, int64_t outf, double dropout, int dtype, int device, int linearized, int gpt_order,
                                          int causal_mask);                                                            /* :492-530; vars (x), tensors (maxLength?) */
int lamp_module_transformer_encoder(lamp_module** out, int64_t num_blocks, int64_t in, int64_t attention_hidden_per_head, int64_t attention_num_heads,
                                    int64_t mlp_hidden, double dropout, int dtype, int device, int linearized, int gpt_order, int causal_mask); /* :76-102 */
int lamp_module_transformer_decoder_block(lamp_module** out, int64_t in, int64_t attention_hidden_per_head, int64_t attention_num_heads,
                                          int64_t mlp_hidden, int64_t outf, double dropout, int dtype, int device, int linearized,
                                          int decoder_decoder_causal_mask, int encoder_decoder_causal_mask);          /* :384-432; vars (decoderInput, encoderOutput), tensors (maxLength?) */
int lamp_module_transformer(lamp_module** out, int64_t num_blocks, int64_t in, int64_t attention_hidden_per_head, int64_t attention_num_heads,
                            int64_t mlp_hidden, double dropout, int dtype, int device, int linearized, int encoder_causal_mask,
                            int decoder_decoder_causal_mask, int encoder_decoder_causal_mask); /* :330-365; vars (decoderInput, encoderInput), tensors (decoderMaxLength?, encoderMaxLength?) */
int lamp_positional_embedding_vaswani(lamp_tensor** out, int64_t sequence_length, int64_t dimension, int dtype, int device); /* :1022-1045 */
int lamp_module_transformer_embedding(lamp_module** out, lamp_module* embedding, int add_positional_embedding,
                                      const lamp_tensor* positional_embedding);                                        /* :1105-1125 */
int lamp_module_language_model(lamp_module** out, int64_t max_length, int64_t vocabulary_size, int64_t num_blocks, int64_t embedding_dim,
                               int64_t attention_hidden_per_head, int64_t attention_num_heads, int64_t encoder_mlp_hidden, double dropout, int dtype,
                               int device, int linearized);                      /* lm.scala:194-232; vars (tokens), tensors (maxLength?, positions?) -> logits */
int lamp_module_language_model_loss(lamp_module** out, int64_t max_length, int64_t vocabulary_size, int64_t num_blocks, int64_t embedding_dim,
                                    int64_t attention_hidden_per_head, int64_t attention_num_heads, int64_t encoder_mlp_hidden, double dropout,
                                    int64_t pad_token, int dtype, int device, int linearized); /* lm.scala:63-91; vars (tokens), tensors (target, maxLength?, positions?) -> loss */
/* LanguageModelOutput(encoded, languageModelLogits) (lm.scala:146-188); either output pointer may be NULL */
int lamp_language_model_forward(lamp_module* m, lamp_var* tokens, const lamp_tensor* max_length_or_null, const lamp_tensor* positions_or_null,
                                lamp_var** encoded, lamp_var** logits);
/* lamp.data.languagemodel.autoregressiveInference (lamp-data languagemodel/package.scala:35-114) for B equal-length prefixes at once.
 * module: a LanguageModelModule or a LanguageModelLoss.  prefix: int64 [B, P], P >= 1, on the model's device or the host.  *tokens:
 * int64 [B, P + length] on the model's device, the prefix followed by what was sampled.  *logits_or_null: the untempered logits of
 * every step, [B, length, V] in the model's type.  Every step sees takeRight(model_block_size) of the sequence at positions
 * 0 .. len - 1; dropout is off during the call and the module's training flags are as before afterwards.  An empty prefix,
 * temperature <= 0 and a model_block_size above the position table are errors.  No step synchronises with the host: the sampled token
 * stays on the device and feeds the next step.
 * With lamp_language_model_decode_fused on (the default), B <= LAMP_DECODE_MAX_ROWS, a model that is not linearized, f32 / f64 / bf16
 * and lamp_attention_fused_call_as_written off: the first window min(P, model_block_size) runs once through the operators of the
 * training forward and fills a key / value cache per block; while the sequence fits model_block_size every further token is one row
 * through the kernels of kernels/decode.hip (5 launches per block + 4); once the window slides every cached position's embedding has
 * moved, so each token is one full forward of the window and lamp_sample_logits.  Otherwise every step is the reference's chain: the
 * full forward, / temperature, logSoftMax, exp, lamp_multinomial. */
int lamp_language_model_generate(lamp_module* module, const lamp_tensor* prefix, int64_t length, double temperature, int64_t model_block_size,
                                 lamp_tensor** tokens, lamp_tensor** logits_or_null);
/* Process-wide; returns the previous value in *previous_or_null. */
int lamp_language_model_decode_fused(int on, int* previous_or_null);
/* which path the calling process's last lamp_language_model_generate took: 1 the decode kernels, 0 the chain, -1 none yet */
int lamp_language_model_generate_path(int* out);
int lamp_sequence_mask(lamp_var** out, const lamp_tensor* max_length, lamp_var* maskable, double fill);   /* MultiheadAttention.sequenceMask :667-749 */
int lamp_masked_softmax(lamp_var** out, lamp_var* input, const lamp_tensor* max_length);                  /* MultiheadAttention.maskedSoftmax :751-762 */
/* ---- BERT pretraining (lamp-core nn/bert/bert.scala).  State order = the reference's `state`: token table, segment table, the positional
 * table (a parameter, [1, max_length, embedding_dim]), the blocks (gptOrder = false, no causal mask), then the masked-language-model
 * decoder (Linear, LayerNorm without scale / bias, Linear) and the whole-sentence classifier (Linear, Linear).  position_embedding_or_null
 * [max_length, embedding_dim]: NULL = PositionalEmbedding.vaswani in single precision, cast to dtype.  per_row_positions (not in the
 * reference): 0 = positions index encoded.view(-1, D) as written (no b * T offset), 1 = every batch row gathers from its own rows. */
int lamp_module_bert_encoder(lamp_module** out, int64_t max_length, int64_t vocabulary_size, int64_t segment_vocabulary_size, int64_t num_blocks,
                             int64_t embedding_dim, int64_t attention_hidden_per_head, int64_t attention_num_heads, int64_t mlp_hidden, double dropout,
                             int dtype, int device, int linearized,
                             const lamp_tensor* position_embedding_or_null);   /* bert.scala:485-534; vars (tokens, segments), tensors (maxLength?) */
int lamp_module_masked_language_model(lamp_module** out, int64_t input_dim, int64_t hidden_dim, int64_t vocabulary_size, int dtype, int device,
                                      int per_row_positions);                   /* :347-359; vars (encoderOutput), tensors (predictionPositions) */
int lamp_module_bert_pretrain(lamp_module** out, int64_t max_length, int64_t vocabulary_size, int64_t segment_vocabulary_size, int64_t mlm_hidden,
                              int64_t whole_sentence_hidden, int64_t num_blocks, int64_t embedding_dim, int64_t attention_hidden_per_head,
                              int64_t attention_num_heads, int64_t encoder_mlp_hidden, double dropout, int dtype, int device, int linearized,
                              const lamp_tensor* position_embedding_or_null,
                              int per_row_positions);   /* :244-285; vars (tokens, segments), tensors (positions, maxLength?) -> language model scores */
int lamp_module_bert_loss(lamp_module** out, int64_t max_length, int64_t vocabulary_size, int64_t segment_vocabulary_size, int64_t mlm_hidden,
                          int64_t whole_sentence_hidden, int64_t num_blocks, int64_t embedding_dim, int64_t attention_hidden_per_head,
                          int64_t attention_num_heads, int64_t encoder_mlp_hidden, double dropout, int64_t pad_token, int dtype, int device,
                          int linearized, const lamp_tensor* position_embedding_or_null,
                          int per_row_positions);   /* :96-140; vars (tokens, segments), tensors (positions, maxLength?, mlmTarget, wholeSentenceTarget) -> loss */
/* BertPretrainOutput(encoded, languageModelScores, wholeSentenceBinaryClassifierScore) (bert.scala:216-228) of a BertPretrainModule or
 * a BertLoss; any output pointer may be NULL */
int lamp_bert_pretrain_forward(lamp_module* m, lamp_var* tokens, lamp_var* segments, const lamp_tensor* positions, const lamp_tensor* max_length_or_null,
                               lamp_var** encoded, lamp_var** language_model_scores, lamp_var** whole_sentence_score);
/* BertEncoder's input embedding as one BertEmbedding node over the kernels of kernels/bert.hip (1) or as the reference's chain of
 * Embedding, Embedding, Add, Slice and Add (0).  Process-wide; returns the previous value in *previous_or_null. */
int lamp_bert_fused(int on, int* previous_or_null);
/* ---- recurrent family (lamp-core nn/RNN.scala, GRU.scala, LSTM.scala, SeqLinear.scala, StatefulSeq.scala).  Inputs [time, batch, in], outputs
 * [time, batch, hidden].  State order = the reference's `state` (LSTM: Xi Xf Xo Hi Hf Ho Xc Hc bI bF bO bC; GRU: Xh Hh Xr Xz Hr Hz bR bZ bH;
 * RNN: Xh Hh bH; SeqLinear: weight, bias).  The plain constructors are the factories (normal(0, sqrt(2 / (fanIn + fanOut))), zero [1, hidden]
 * biases); the _from forms are the case classes' constructors over the caller's tensors in that order (biases [hidden] or [1, hidden]). */
int lamp_module_rnn(lamp_module** out, int64_t in, int64_t hidden, int dtype, int device);
int lamp_module_gru(lamp_module** out, int64_t in, int64_t hidden, int dtype, int device);
int lamp_module_lstm(lamp_module** out, int64_t in, int64_t hidden, int dtype, int device);
int lamp_module_seq_linear(lamp_module** out, int64_t in, int64_t outf, int dtype, int device);
int lamp_module_rnn_from(lamp_module** out, const lamp_tensor* const* tensors, int n);
int lamp_module_gru_from(lamp_module** out, const lamp_tensor* const* tensors, int n);
int lamp_module_lstm_from(lamp_module** out, const lamp_tensor* const* tensors, int n);
int lamp_module_seq_linear_from(lamp_module** out, const lamp_tensor* const* tensors, int n);
/* statefulSequence(m1, ..., mn): stateless members (Embedding, Fun, SeqLinear) are lifted; the state is the members' states side by side */
int lamp_module_stateful_sequence(lamp_module** out, lamp_module* const* mods, int n);
/* number of Variables in a stateful module's state: LSTM 2 (h, c), GRU / RNN 1, a stateful sequence the sum over its members; FreeRunningRNN
 * and WithInit their module's, Seq2Seq its encoder's */
int lamp_module_num_state_slots(lamp_module* m, int* out);
/* StatefulModule.forward((x, state)): `state` holds nstate Variables (NULL entries, or nstate = 0: the reference's None - zeros); returns the
 * output and the next state (state_out: capacity lamp_module_num_state_slots, +1 handles).  Gradients flow through the returned state. */
int lamp_module_forward_stateful(lamp_module* m, lamp_var* x, lamp_var* const* state, int nstate, lamp_var** out, lamp_var** state_out);
/* RNN / GRU / LSTM / SeqLinear as one node per sequence over the fused cell kernels (1, the default unless LAMP_RECURRENT_FUSED=0) or as the
 * reference's fold over the time steps built from the plain operators (0).  Process-wide; returns the previous value in *previous_or_null. */
int lamp_recurrent_fused(int on, int* previous_or_null);
/* ---- recurrent text generation (lamp-core nn/FreeRunningRNN.scala, nn/Seq2Seq.scala; lamp-data Text.scala:18-135) ----
 * FreeRunningRNN(module, time_steps): a stateful module; forward((x [T0, B] int64, state)) = (outputs [time_steps, B, V], lastState): the
 * first iteration forwards the whole prefix, every further one the detached argmax(2) of the last time step, [1, B].  A composition of the
 * wrapped module's own nodes, so gradients flow through outputs and state.  state / training mode / slots are the wrapped module's. */
int lamp_module_free_running_rnn(lamp_module** out, lamp_module* module, int64_t time_steps);
/* Seq2Seq(encoder, decoder): forward(((source, dest), state0)) = decoder.forward((dest, encoder.forward((source, state0)).state)) through
 * lamp_module_forward_stateful_pair; state = encoder.state ++ decoder.state; the encoder's state is the decoder's initial state, so both have
 * the same number of slots. */
int lamp_module_seq2seq(lamp_module** out, lamp_module* encoder, lamp_module* decoder);
/* WithInit(module, init): the module with an initial state of its own, n = lamp_module_num_state_slots(module) Variables */
int lamp_module_with_init(lamp_module** out, lamp_module* module, lamp_var* const* init, int n);
/* InitState: *n = 0 for the reference's None (RNN, GRU, LSTM, statefulSequence), the carried Variables for WithInit (+1 handles, capacity
 * lamp_module_num_state_slots); FreeRunningRNN answers with its module's, Seq2Seq with its encoder's */
int lamp_module_init_state(lamp_module* m, lamp_var** out, int* n);
/* lamp_module_forward_stateful for a module whose input is a pair of Variables (Seq2Seq: source, dest) */
int lamp_module_forward_stateful_pair(lamp_module* m, lamp_var* x0, lamp_var* x1, lamp_var* const* state, int nstate, lamp_var** out, lamp_var** state_out);
/* Text.sequencePrediction: FreeRunningRNN(module, steps).forward((prefix, module.initState)), values only.  prefix: int64 [T0, B] on the
 * module's device.  *tokens: int64 [steps, B], the argmax(2) of *outputs_or_null [steps, B, V].
 * With lamp_text_generation_fused on, a module of the shape statefulSequence(Embedding, one of RNN | GRU | LSTM, [Fun relu], SeqLinear,
 * [Fun logsoftmax over dimension 2]) (possibly inside WithInit), f32 or f64 on a device and B <= LAMP_DECODE_MAX_ROWS: the prefix runs once
 * through the module's own forward, then every token is lamp_recurrent_decode_step (GRU: two launches), lamp_decode_linear and
 * lamp_log_softmax_argmax_rows; the token stays on the device.  Anything else runs the chain above. */
int lamp_text_sequence_prediction(lamp_module* module, const lamp_tensor* prefix, int64_t steps, lamp_tensor** tokens, lamp_tensor** outputs_or_null);
/* Text.sequencePredictionBeam (Text.scala:38-135) for one prefix [T0, 1]: up to k sequences, best first.  Sequence i is
 * tokens_out[offsets_out[i] .. offsets_out[i + 1]) (it starts with the prefix's last token and has at most steps + 1 entries; a beam whose
 * last token is end_of_sequence is carried unchanged) with log-probability log_probs_out[i], summed in double on the host.  Capacities:
 * tokens_out k * (steps + 1), offsets_out k + 1, log_probs_out k.  Per step the live beams are one batch (fused: their states gathered by
 * the step kernel's parent argument), a sorted per-row lamp_topk and ONE host read; the fused path needs k <= LAMP_DECODE_MAX_ROWS. */
int lamp_text_sequence_prediction_beam(lamp_module* module, const lamp_tensor* prefix, int64_t steps, int64_t start_sequence, int64_t end_of_sequence,
                                       int64_t k, int64_t* tokens_out, int64_t* offsets_out, double* log_probs_out, int* num_sequences);
/* Process-wide, run-time only; returns the previous value in *previous_or_null. */
int lamp_text_generation_fused(int on, int* previous_or_null);
/* which path the calling process's last sequence prediction took: 1 the decode kernels, 0 the chain, -1 none yet */
int lamp_text_generate_path(int* out);
/* GenericModule[A, B].forward for a tuple / case-class A: its Variables and its plain tensors in the reference's order; a NULL tensor = None */
int lamp_module_forward_multi(lamp_module* m, lamp_var* const* vars, int nvars, const lamp_tensor* const* tensors, int ntensors, lamp_var** out);
int lamp_module_forward(lamp_module* m, lamp_var* x, lamp_var** out);
int lamp_module_num_state(lamp_module* m, int64_t* out);
int lamp_module_state(lamp_module* m, int64_t index, lamp_var** out);   /* state in lamp's order (params and consts) */
int lamp_module_set_training(lamp_module* m, int training);              /* asTraining / asEval */
int lamp_module_zero_grad(lamp_module* m);
int lamp_module_release(lamp_module* m);

/* ---- optimisers (nn/AdamW.scala, nn/SGD.scala); clip < 0 means None ---- */
int lamp_optimizer_adamw(lamp_optimizer** out, lamp_tensor* const* params, int n, double weight_decay, double learning_rate, double beta1,
                         double beta2, double eps, double clip, int debias, int mixed_precision);
/* AdamW with OptimizedHyperparameter = PTag => Double resolved per parameter (AdamW.scala:29-47, train.scala:48-66 of
 * example-autoregressivelm: weight decay on the attention / MLP matrices only): arrays of n values */
int lamp_optimizer_adamw_tagged(lamp_optimizer** out, lamp_tensor* const* params, int n, const double* weight_decay, const double* learning_rate,
                                const double* beta1, const double* beta2, double eps, double clip, int debias, int mixed_precision);
int lamp_optimizer_sgdw(lamp_optimizer** out, lamp_tensor* const* params, int n, double learning_rate, double weight_decay,
                        double momentum /* < 0: none */, double clip);
/* nn/RAdam.scala, nn/Yogi.scala: arrays of n values (OptimizerHyperparameter resolved per parameter); state = [stepCount] ++ mt ++ vt.
 * Yogi.step overwrites the gradient tensors it is handed (Yogi.scala:95-98). */
int lamp_optimizer_radam(lamp_optimizer** out, lamp_tensor* const* params, int n, const double* weight_decay, const double* learning_rate,
                         const double* beta1, const double* beta2, double eps, double clip);
int lamp_optimizer_yogi(lamp_optimizer** out, lamp_tensor* const* params, int n, const double* weight_decay, const double* learning_rate,
                        const double* beta1, const double* beta2, double eps, double clip, int debias);
/* nn/Shampoo.scala: learning_rate / momentum hold n values; state = [stepCount] ++ (lt, ltinv)* ++ (rt, rtinv)* ++ lastGradient.
 * With momentum > 0 step overwrites the gradient tensors it is handed (Shampoo.scala:107-110).  paper_preconditioner is not in the
 * reference: the stored inverse roots are U diag(s^-1/4) U^T instead of the diagonal matrix the reference computes. */
int lamp_optimizer_shampoo(lamp_optimizer** out, lamp_tensor* const* params, int n, const double* learning_rate, double clip, double eps,
                           int64_t update_preconditioner_every_n_iterations, const double* momentum, int paper_preconditioner);
int lamp_optimizer_step(lamp_optimizer* o, lamp_tensor* const* gradients /* NULL entries = None */, int n, double schedule_factor);
int lamp_optimizer_num_state(lamp_optimizer* o, int64_t* out);
int lamp_optimizer_state(lamp_optimizer* o, int64_t index, lamp_tensor** out);
/* Optimizer.load (AdamW.scala:87-93, SGD.scala:38-42): copyFrom into the state tensors in order; AdamW re-reads its step count */
int lamp_optimizer_load(lamp_optimizer* o, lamp_tensor* const* tensors, int n);
int lamp_optimizer_release(lamp_optimizer* o);
/* nn/package.scala:72-100 */
int lamp_gradient_clipping_in_place(lamp_tensor* const* gradients, int n, double theta);

/* ---- supervised model + training steps ---- */
/* loss_kind 0: LossFunctions.NLL(numClasses, classWeights, reduction, ignore) ; 1: MSE ; 2: Identity ;
 * 3: SequenceNLL(numClasses, classWeights, ignore) over outputs [time, batch, classes] and targets [time, batch] (LossFunctions.scala:76-108) */
int lamp_model_create(lamp_model** out, lamp_module* module, int loss_kind, const lamp_tensor* class_weights_or_null, int64_t reduction,
                      int64_t ignore_index);
/* SupervisedModel.addTotalLossAndReturnGradientsAndNumExamples (SupervisedModel.scala:190-211):
 * forward, loss, zero grads, backprop; acc += loss * n. Gradients are left in the parameters' grad buffers. */
int lamp_model_gradients(lamp_model* m, const lamp_tensor* samples, const lamp_tensor* target, lamp_tensor* acc_or_null, int zero_grad,
                         int64_t* num_examples);
int lamp_model_forward_loss(lamp_model* m, const lamp_tensor* samples, const lamp_tensor* target, lamp_tensor* acc_or_null,
                            int64_t* num_examples);
/* one full step = gradients + (optional RCCL exchange) + optimizer.step, as IOLoops.oneEpoch's processBatch
 * (lamp-data/.../IOLoops.scala:621-658) or distributed oneBatch (distributed/package.scala:733-759) */
int lamp_model_train_step(lamp_model* m, lamp_optimizer* o, lamp_comm* comm_or_null, const lamp_tensor* samples, const lamp_tensor* target,
                          lamp_tensor* acc_or_null, int64_t* num_examples);
/* the same with the learning-rate schedule factor of the epoch (IOLoops.scala:621-658 `learningRateScheduleFactor`) */
int lamp_model_train_step_scheduled(lamp_model* m, lamp_optimizer* o, lamp_comm* comm_or_null, const lamp_tensor* samples,
                                    const lamp_tensor* target, lamp_tensor* acc_or_null, double schedule_factor, int64_t* num_examples);
/* broadcast of module.state (parameters and batch-norm running statistics) and the optimiser state from `root` to every rank
 * (distributed/package.scala:683-688).  lamp_model_train_step does it by itself before the first step over a communicator; call it
 * again before validation / checkpoints to make rank `root`'s non-parameter state the state of every rank. */
int lamp_model_sync_state(lamp_model* m, lamp_optimizer* o, lamp_comm* comm, int root);
/* averageGradients + optimizer.step (distributed/package.scala:690-759) on gradients the caller has already computed - e.g. by replaying
 * forward + backprop from a HIP graph: g_i *= n, one flat all-reduce with n, g_i /= sum n, step.  The replicas are made identical first
 * if they have not been over this communicator. */
int lamp_model_exchange_and_step(lamp_model* m, lamp_optimizer* o, lamp_comm* comm, lamp_tensor* const* grads, int ngrads, int64_t num_examples,
                                 double schedule_factor);
/* Single-process data parallel, DataParallel.driveSynchronousLoop's `synchronousStep` (lamp-data DataParallel.scala:195-311): the main
 * model (with the optimiser) and `nreplicas` replicas on other GPUs; arrays of nreplicas + 1 entries, main first.  Copies the main
 * state to the replicas, computes every model's gradients on its own host thread, and - when `step` - averages the gradients weighted
 * by the example counts into the main model and steps the optimiser.  Returns the examples of all models. */
int lamp_data_parallel_step(lamp_model* main_model, lamp_optimizer* o, lamp_model* const* replicas, int nreplicas, const lamp_tensor* const* samples,
                            const lamp_tensor* const* targets, lamp_tensor* const* accs_or_null, int zero_grad, int step, double schedule_factor,
                            int64_t* num_examples);
int lamp_model_release(lamp_model* m);

/* ---- tensor-list files and checkpoints (lamp-data Writer.scala:14-190, Reader.scala:17-95, schemas.scala:30-56) ----
 * A list of tensors is a JSON descriptor {"tensors":[{"dims","dataType","byteOffset","byteLength"}...],"location",
 * "byteOffset","byteLength"} at `path` plus the raw little-endian blob `path`.data (every tensor padded to a multiple
 * of 8 bytes); `location` is relative to the descriptor unless absolute.  Files written here are readable by the
 * reference's Reader and the other way round. */
int lamp_write_tensors_into_file(lamp_tensor* const* tensors, int64_t n, const char* path);    /* Writer.writeTensorsIntoFile */
int lamp_tensor_list_length(const char* path, int64_t* n);
/* Reader.readTensorsFromFile(file, device, pin) with STen.tensorsFromFile's checks (STen.scala:157-168); device -1 = host */
int lamp_read_tensors_from_file(lamp_tensor** out /* capacity */, int64_t capacity, int64_t* n_read, const char* path, int device, int pin);
int lamp_module_write_checkpoint(lamp_module* m, const char* path);     /* Writer.writeCheckpoint: module.state in order */
int lamp_module_load_from_file(lamp_module* m, const char* path);       /* Reader.loadFromFile: copyFrom per state tensor */

/* Cifar.loadImageFile (example-cifar100/.../cifar100.scala:29-56): records of 3074 bytes (coarse label, fine label,
 * 3x32x32 pixels); labels = i64 fine labels [n], images = [n, 3, 32, 32] cast to `dtype` (raw 0..255 values). */
int lamp_cifar_load_image_file(lamp_tensor** labels, lamp_tensor** images, const char* path, int64_t num_images, int dtype, int device);

/* ---- BatchStream.minibatchesFromFull (BatchStream.scala:528-592) + everyNth (:378-400) ----
 * `order` is the shuffled row order (the caller owns the RNG: scala.util.Random.shuffle on the JVM); it is cut into groups of
 * minibatch_size; drop_last removes the LAST group whether or not it is full, as the reference does.  The data set lives in
 * HBM and a minibatch is one gather on the device.  next: *x = NULL at EndStream. */
typedef struct lamp_batch_stream lamp_batch_stream;
int lamp_batch_stream_from_full(lamp_batch_stream** out, const lamp_tensor* features, const lamp_tensor* target, const int64_t* order, int64_t n,
                                int64_t minibatch_size, int drop_last, int device);
/* The same stream over a data set that STAYS IN HOST MEMORY, as in the reference (BatchStream.scala:539-556: host gather, pinned staging buffer,
 * copy on another stream; `pinned` of cifar100.scala): the features are pinned (copied once if they are not), and the GPU gathers a
 * minibatch's rows over PCIe, queued one batch ahead of the consumer (IOLoops.scala:833-874), converting to out_dtype (-1: as
 * stored) on the way.  Batches, order and values are those of lamp_batch_stream_from_full. */
int lamp_batch_stream_from_full_host(lamp_batch_stream** out, const lamp_tensor* features, const lamp_tensor* target, const int64_t* order, int64_t n,
                                     int64_t minibatch_size, int drop_last, int device, int out_dtype);
int lamp_batch_stream_every_nth(lamp_batch_stream* s, int64_t n, int64_t offset);
int lamp_batch_stream_num_batches(const lamp_batch_stream* s, int64_t* out);
int lamp_batch_stream_next(lamp_batch_stream* s, lamp_tensor** x, lamp_tensor** target);
int lamp_batch_stream_reset(lamp_batch_stream* s);
int lamp_batch_stream_release(lamp_batch_stream* s);

#ifdef __cplusplus
}
#endif
#endif /* LAMP_HOST_H */
