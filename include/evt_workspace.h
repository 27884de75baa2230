/* Companion of evt.h (which includes it): what a live handle's workspace takes.
 * Same conventions: C ABI of libevt_hip.so, EVT_* return codes, evt_last_error() for the text. */
#ifndef EVT_WORKSPACE_H_
#define EVT_WORKSPACE_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

struct evt_model;

/* Bytes the handle's workspace allocations asked for, its lane children's included: what
 * evt_*_query_workspace returns for the handle's max_batch and, with k lanes
 * (evt_model_set_lanes), k times what it returns for ceil(max_batch / k) on top. The weights are
 * not counted. EVT_EINVAL on a NULL argument. */
int evt_model_workspace_bytes(const struct evt_model* m, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* EVT_WORKSPACE_H_ */
