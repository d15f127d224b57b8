// A/B build of csrc/qstep_ws.hip: tick reciprocals by IEEE division at the head of the features (the form before WS_TICK_RCP / WS_TICK_HOIST).
#define WS_TICK_RCP 0
#define WS_TICK_HOIST 0
#define WS_NS ws_tickrcp0
#define WS_API(name) name##_tickrcp0
#include "../qstep_ws.hip"
