// fq_embed.h -- pooled text vectors: the arithmetic of the mean over the ln_f rows of a text and of its L2 normalisation, restated once
// for the device (kernels_embed.hip) and the numpy statement the tests hold it against (tests/embed_ref.py):
//   acc[col]  = a double that starts at 0 and takes (double) row[i][col] for the rows i = 0, 1, ... of every call since the last reset IN THAT ORDER;
//   mean[col] = (float)(acc[col] / (double) count);
//   s         = the sum of (double) mean[col] * (double) mean[col] (each product is exact in f64): thread t of FQ_EMBED_THREADS chains the columns
//               t, t + FQ_EMBED_THREADS, ... upwards from 0.0, and the partials are chained in thread order upwards from 0.0;
//   out[col]  = (float)((double) mean[col] / sqrt(s)).
// The order of acc's chain is the contract (2^60, 1, -2^60 gives 0 in this order and 1 in another): one lane owns a column, rows are never
// split over workgroups. s has one fixed order as well, so a vector is the same from run to run.
#pragma once
#include "fq_types.h"

#define FQ_EMBED_THREADS 256        // workgroup of the finishing launch = the stride of s's partial chains

FQ_HD double fq_embed_step(double acc, float v) { return acc + (double) v; }             // one link of a column's chain
FQ_HD float  fq_embed_mean(double acc, long long count) { return (float)(acc / (double) count); }
FQ_HD double fq_embed_sq_step(double s, float mean) { return s + (double) mean * (double) mean; }
FQ_HD float  fq_embed_unit(float mean, double root) { return (float)((double) mean / root); }
