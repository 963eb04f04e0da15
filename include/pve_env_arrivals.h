/* pve_env_arrivals.h -- extension of the C ABI of pve_env.h (libpveenv.so, ABI 9): the arrival generator's entry point.
 * The struct pve_arrival_gen, the word layout, the arithmetic and the errors are documented in pve_env.h ("ARRIVAL STREAMS generated
 * on the device"); the specification is csrc/pve_arrivals.h.  A library older than this header lacks the symbol. */
#ifndef PVE_ENV_ARRIVALS_H
#define PVE_ENV_ARRIVALS_H

#include "pve_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces the loadmat of main.py:228-229 / :388-389 and, for lane_num = 8, the intention draws of ref :381, :390.  Asynchronous on
 * the handle's stream; does not install the stream (pve_set_arrivals / pve_set_intentions do). */
int pve_generate_arrivals(pve_handle h, const pve_arrival_gen *g, double *arrivals /* DEVICE, 16-byte aligned */,
                          int32_t *intentions /* or NULL */, double *covered /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PVE_ENV_ARRIVALS_H */
