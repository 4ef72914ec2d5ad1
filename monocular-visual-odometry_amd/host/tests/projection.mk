# host/tests/projection.mk -- test_projection_match: the mirror of tracking by projection (my_slam/vo/projection_match.h) and
# the poseEstimationPnP that can use it, written against the reference-shaped headers and linked to libmvo_hip.so only
# (tests/test_projection_host.py runs it on the MI355X and, with the emulated build in front of the library search path, on
# the CPU).
#   make -C host/tests -f projection.mk
include Makefile
projection: test_projection_match
test_projection_match: test_projection_match.cpp $(DROPIN) $(wildcard ../include/my_slam/*.h ../include/my_slam/*/*.h) $(ROOT)/include/mvo_hip.h
	$(CXX) $(CXXFLAGS) -o $@ test_projection_match.cpp $(DROPIN) -L$(LIBDIR) -lmvo_hip -Wl,-rpath,'$$ORIGIN/../../csrc' -Wl,-rpath,/opt/rocm/lib
.DEFAULT_GOAL := projection
.PHONY: projection
