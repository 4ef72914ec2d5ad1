# host/tests/map_refine.mk -- test_map_refine: the mirror of the map-point position refinement (my_slam/vo/map_refine.h), written
# against the reference-shaped headers and linked to libmvo_hip.so only (tests/test_map_refine_host.py runs it on the MI355X and,
# with the emulated build in front of the library search path, on the CPU).
#   make -C host/tests -f map_refine.mk
include Makefile
map_refine: test_map_refine
test_map_refine: test_map_refine.cpp $(DROPIN) $(wildcard ../include/my_slam/*.h ../include/my_slam/*/*.h) $(ROOT)/include/mvo_hip.h
	$(CXX) $(CXXFLAGS) -o $@ test_map_refine.cpp $(DROPIN) -L$(LIBDIR) -lmvo_hip -Wl,-rpath,'$$ORIGIN/../../csrc' -Wl,-rpath,/opt/rocm/lib
.DEFAULT_GOAL := map_refine
.PHONY: map_refine
