// A/B build of csrc/qstep_ws.hip: the cheaper tick reciprocal, formed at the head of the features (not hoisted to the end of the previous tile).
#define WS_TICK_HOIST 0
#define WS_NS ws_tickhoist0
#define WS_API(name) name##_tickhoist0
#include "../qstep_ws.hip"
