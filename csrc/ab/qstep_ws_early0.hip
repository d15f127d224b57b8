// A/B build of csrc/qstep_ws.hip: tile 0's loads issued after the weight-image copy and the barrier (the form before WS_EARLY_LOADS).
#define WS_EARLY_LOADS 0
#define WS_NS ws_early0
#define WS_API(name) name##_early0
#include "../qstep_ws.hip"
