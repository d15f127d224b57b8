// A/B build of csrc/qstep_ws.hip: the gradient waves read dZ1's W1^T fragments inside the phase, after the wait for the slot pair.
#define WS_GW1PRE 0
#define WS_NS ws_gw1pre0
#define WS_API(name) name##_gw1pre0
#include "../qstep_ws.hip"
