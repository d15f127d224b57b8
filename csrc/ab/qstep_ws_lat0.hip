// A/B build of csrc/qstep_ws.hip: none of the four latency items (the schedule before profiles/ws_latency_items.md).
#define WS_L2NPRE 0
#define WS_GW1PRE 0
#define WS_TICK_RCP 0
#define WS_TICK_HOIST 0
#define WS_EARLY_LOADS 0
#define WS_NS ws_lat0
#define WS_API(name) name##_lat0
#include "../qstep_ws.hip"
