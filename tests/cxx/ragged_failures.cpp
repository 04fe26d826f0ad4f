// ragged_failures.cpp -- the first-failure rule of the list reconstruction calls (libjpeg_amd/csrc/ragged_failures.hpp) as a program
// of its own, for the sanitizers: codes and messages against the texts written out here.  No device, nothing of the library is linked.
// (tests/test_ragged_twin_cpu.py builds it with -fsanitize=address,undefined and runs it.)
#include <stdio.h>

#include <string>

#include "ragged_failures.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      failures++;                                                          \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond);     \
    }                                                                      \
  } while (0)

// what finish() reports to: the decoder object's error, as set_error (decoder.hpp) keeps it
struct Object {
  int err_code = 0;
  std::string err_msg;
};
static int set_error(Object *o, int code, const std::string &msg)
{
  o->err_code = code;
  o->err_msg = msg;
  return code;
}

int main()
{
  { // no failure: MIJPEG_OK, and the object's error is left alone
    RaggedFailures f;
    Object o;
    o.err_code = -7;
    o.err_msg = "an earlier call's";
    f.note(3, MIJPEG_OK);
    f.note(4, MIJPEG_OK, "a child's text that nobody asked for");
    CHECK(f.code == MIJPEG_OK && f.message.empty());
    CHECK(f.finish(&o) == MIJPEG_OK);
    CHECK(o.err_code == -7 && o.err_msg == "an earlier call's");
  }
  { // images 5, 2 and 7 fail in that order: the first noted failure wins, not the lowest index and not the last
    RaggedFailures f;
    Object o;
    f.note(0, MIJPEG_OK);
    f.note(5, MIJPEG_ERR_DEVICE);
    f.note(2, MIJPEG_ERR_INVALID_PARAMETER, "the child of image 2");
    f.note(7, MIJPEG_ERR_NOT_IMPLEMENTED, "");
    CHECK(f.code == MIJPEG_ERR_DEVICE);
    CHECK(f.message == "image 5 of the ragged batch was not reconstructed");
    CHECK(f.finish(&o) == MIJPEG_ERR_DEVICE);
    CHECK(o.err_code == MIJPEG_ERR_DEVICE && o.err_msg == "image 5 of the ragged batch was not reconstructed");
  }
  { // a child object's message follows behind ": "
    RaggedFailures f;
    Object o;
    f.note(12, MIJPEG_ERR_NOT_IMPLEMENTED, "reconstruction not available for this stream");
    CHECK(f.code == MIJPEG_ERR_NOT_IMPLEMENTED);
    CHECK(f.message == "image 12 of the ragged batch was not reconstructed: reconstruction not available for this stream");
    CHECK(f.finish(&o) == MIJPEG_ERR_NOT_IMPLEMENTED && o.err_msg == f.message);
  }
  { // a child without a text (the full and planar calls pass "" then): the message ends in ": "
    RaggedFailures f;
    f.note(0, MIJPEG_ERR_DEVICE, "");
    CHECK(f.message == "image 0 of the ragged batch was not reconstructed: ");
  }
  { // no detail at all (the object's own launches, the crop call's copy route): no suffix
    RaggedFailures f, g;
    f.note(2147483647, MIJPEG_ERR_DEVICE, nullptr);
    CHECK(f.message == "image 2147483647 of the ragged batch was not reconstructed");
    g.note(1, MIJPEG_ERR_DEVICE);
    CHECK(g.message == "image 1 of the ragged batch was not reconstructed");
  }
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("OK ragged_failures\n");
  return 0;
}
