// fq_lora_base.h -- how the LoRA merge (falcon_model.hip, which owns the model) reaches the tensors of a base model file (falcon_ggcc.hip, which owns the
// GGCC reader): falcon_hip_model_apply_lora opens the file and hands the merge a lookup. Internal to libggml_hip.so.
#pragma once
#include <stdint.h>

struct falcon_hip_model;
struct fq_lora_base_tensor { bool found; int type, n_dims; int64_t ne0, ne1; const uint8_t * data; };      // data: host bytes in the file's (ggml) layout
typedef fq_lora_base_tensor (*fq_lora_base_fn)(void * user, const char * name);
// base == nullptr: no base file (the model's own rows are patched)
int fq_model_apply_lora(falcon_hip_model * m, const char * path_lora, fq_lora_base_fn base, void * user);
