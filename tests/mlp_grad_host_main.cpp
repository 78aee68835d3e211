// Stand-alone check of be_mlp_grad's host logic in csrc/host_logic.h (no HIP): the shape bounds, the
// w3 / b3 rule and the layout of a workgroup's workspace slot.  Built and run by
// tests/test_mlp_grad_host.py under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <stdio.h>
#include <string.h>

#include "host_logic.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);             \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static bool says(const char* msg, const char* word) { return msg && strstr(msg, word); }

int main() {
  using namespace behost;
  CHECK(!mlp_grad_shape_error(3, 128, 128, 9) && !mlp_grad_shape_error(2, 128, 0, 9));
  CHECK(!mlp_grad_shape_error(3, 1, 1, 1) && !mlp_grad_shape_error(2, 1, 0, 15));
  CHECK(says(mlp_grad_shape_error(1, 128, 0, 9), "layers") && says(mlp_grad_shape_error(4, 128, 128, 9), "layers"));
  CHECK(says(mlp_grad_shape_error(3, 0, 128, 9), "hidden1") && says(mlp_grad_shape_error(3, 129, 128, 9), "hidden1"));
  CHECK(says(mlp_grad_shape_error(3, 128, 0, 9), "hidden2") && says(mlp_grad_shape_error(3, 128, 129, 9), "hidden2"));
  CHECK(says(mlp_grad_shape_error(2, 128, 128, 9), "hidden2"));
  CHECK(says(mlp_grad_shape_error(2, 128, 0, 0), "num_actions") && says(mlp_grad_shape_error(2, 128, 0, 16), "num_actions"));
  int x = 0;
  CHECK(!mlp_grad_last_layer_error(3, &x, &x) && !mlp_grad_last_layer_error(2, nullptr, nullptr));
  CHECK(says(mlp_grad_last_layer_error(3, nullptr, &x), "w3") && says(mlp_grad_last_layer_error(3, &x, nullptr), "w3"));
  CHECK(says(mlp_grad_last_layer_error(2, &x, nullptr), "w3") && says(mlp_grad_last_layer_error(2, nullptr, &x), "w3"));

  // the slot: the tensors in state_dict order, back to back, then two 8-byte aligned f64
  const MlpGradSlot a = mlp_grad_slot(3, 128, 128, 9);
  CHECK(a.o_b1 == 128 * 29 && a.o_w2 == a.o_b1 + 128 && a.o_b2 == a.o_w2 + 128 * 128 && a.o_w3 == a.o_b2 + 128);
  CHECK(a.o_b3 == a.o_w3 + 9 * 128 && a.P == a.o_b3 + 9 && a.P == 21513);
  CHECK(a.loss_off % 8 == 0 && a.loss_off >= 4 * a.P && a.loss_off < 4 * a.P + 8 && a.slot_bytes == a.loss_off + 16);
  const MlpGradSlot b = mlp_grad_slot(2, 100, 0, 5);
  CHECK(b.o_b1 == 2900 && b.o_w2 == 3000 && b.o_b2 == 3500 && b.o_w3 == 3505 && b.o_b3 == 3505 && b.P == 3505);
  CHECK(b.loss_off == 14024 && b.slot_bytes == 14040 && b.slot_bytes % 8 == 0);
  const MlpGradSlot c = mlp_grad_slot(3, 17, 128, 15);
  CHECK(c.P == 17 * 29 + 17 + 128 * 17 + 128 + 15 * 128 + 15 && c.slot_bytes % 8 == 0);
  printf("mlp_grad_host: OK\n");
  return 0;
}
