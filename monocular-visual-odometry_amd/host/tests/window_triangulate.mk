# host/tests/window_triangulate.mk -- test_window_triangulate: the mirror of the new map points from every buffered frame
# (my_slam/vo/window_triangulate.h), written against the reference-shaped headers and linked to libmvo_hip.so only
# (tests/test_window_triangulate_host.py runs it on the MI355X and, with the emulated build in front of the library search path,
# on the CPU).
#   make -C host/tests -f window_triangulate.mk
include Makefile
window_triangulate: test_window_triangulate
test_window_triangulate: test_window_triangulate.cpp $(DROPIN) $(wildcard ../include/my_slam/*.h ../include/my_slam/*/*.h) $(ROOT)/include/mvo_hip.h
	$(CXX) $(CXXFLAGS) -o $@ test_window_triangulate.cpp $(DROPIN) -L$(LIBDIR) -lmvo_hip -Wl,-rpath,'$$ORIGIN/../../csrc' -Wl,-rpath,/opt/rocm/lib
.DEFAULT_GOAL := window_triangulate
.PHONY: window_triangulate
