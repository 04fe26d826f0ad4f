// ragged_failures.hpp -- the first-failure rule of the list reconstruction calls (ragged_reconstruct.cpp, reconstruct_planar_items):
// one picture whose reconstruction fails does not stop the others, whichever route it takes; the call works through the list and
// then returns the first such code, with a message that names the image.  (A whole launch that fails is the device's failure and
// ends the call at once.)  Calls nothing of the HIP runtime: tests/cxx/ragged_failures.cpp is built around it.  Private to libmijpeg.so.
#pragma once
#include <string>
#include "../../include/mijpeg.h"

struct RaggedFailures {
  int code = MIJPEG_OK;
  std::string message;
  // Image `image` ended with rc.  detail: the message of the child object that reconstructed it ("" where it has none: the ": " of a
  // child's report stays), nullptr: the failure is this object's own, no suffix.
  void note(int image, int rc, const char *detail = nullptr)
  {
    if (!rc || code) return;
    code = rc;
    message = "image " + std::to_string(image) + " of the ragged batch was not reconstructed";
    if (detail) message.append(": ").append(detail);
  }
  // What the call returns: MIJPEG_OK, or the first failure as the error of d (set_error, decoder.hpp)
  template <class Decoder> int finish(Decoder *d) const { return code ? set_error(d, code, message) : MIJPEG_OK; }
};
