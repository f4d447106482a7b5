/* mm_dense_host.h -- the former name of mm_metric_host.h, which holds mm_tri_len and mm_dense_prepare unchanged; kept so that a
 * host program written against this name still builds.  New code includes mm_metric_host.h. */
#include "mm_metric_host.h"
