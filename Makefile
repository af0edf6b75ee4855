# gpusort-mi355x — build the C-ABI library (gfx950 only) and the CPU oracle.
HIPCC ?= hipcc
HIPFLAGS ?= --offload-arch=gfx950 -O3 -std=c++17 -fPIC
LIBDIR := gpusorting_amd/lib
LIB := $(LIBDIR)/libgpusort.so
SRC := gpusorting_amd/csrc/gpusort_capi.hip
# one translation unit: every header under csrc/ is part of it
HDR := $(wildcard gpusorting_amd/csrc/*.hpp) include/gpusort.h
# The four library flavours, name -> extra flags.  The fault-injection builds: one tile withholds its descriptor, short spin bounds
# (with the look-back fallback the sort must still be exact, without it it must report GS_ERR_TIMEOUT and write nothing wrong).
# The tuning build: calibration kernels + tuning tile shapes (u32 keys-only kernels only: a 10 s compile); tools/ and bench.py's box_floor block.
FLAVOURS := libgpusort libgpusort_fault libgpusort_fault_nofallback libgpusort_tuning
FLAGS_libgpusort :=
FLAGS_libgpusort_fault := -DGS_EXP=8 -DGS_FALLBACK_SPINS=4096 -DGS_MID_ADOPT_SPINS=4
FLAGS_libgpusort_fault_nofallback := -DGS_EXP=8 -DGS_FALLBACK=0 -DGS_SPIN_LIMIT=4096
FLAGS_libgpusort_tuning := -DGS_MINIMAL -DGS_TUNING
LIBS := $(FLAVOURS:%=$(LIBDIR)/%.so)

all: libs oracle tools
libs: $(LIBS)
$(LIBS): $(LIBDIR)/%.so: $(SRC) $(HDR)
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared $(FLAGS_$*) $(SRC) -o $@
oracle:
	$(MAKE) -C oracle
tools: build/gpusorting_main build/gpusorting_d3d12_main build/rocprim_compare build/mgpu_main
build/mgpu_main: tools/mgpu_main.cpp include/gpusort.h $(LIB)
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -Iinclude tools/mgpu_main.cpp -Lgpusorting_amd/lib -lgpusort -lpthread -Wl,-rpath,'$$ORIGIN/../gpusorting_amd/lib' -o $@
build/gpusorting_d3d12_main: tools/gpusorting_d3d12_main.cpp include/gpusort/GPUSortBase.hpp $(LIB)
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -Iinclude tools/gpusorting_d3d12_main.cpp -Lgpusorting_amd/lib -lgpusort -Wl,-rpath,'$$ORIGIN/../gpusorting_amd/lib' -o $@
build/gpusorting_main: tools/gpusorting_main.cpp include/gpusort/OneSweepDispatcher.hpp $(LIB)
	@mkdir -p build
	$(HIPCC) -O2 -std=c++17 -Iinclude tools/gpusorting_main.cpp -Lgpusorting_amd/lib -lgpusort -Wl,-rpath,'$$ORIGIN/../gpusorting_amd/lib' -o $@
build/rocprim_compare: tools/rocprim_compare.cpp $(LIB)
	@mkdir -p build
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -Iinclude tools/rocprim_compare.cpp -Lgpusorting_amd/lib -lgpusort -Wl,-rpath,'$$ORIGIN/../gpusorting_amd/lib' -o $@
clean:
	rm -rf build $(LIBS); $(MAKE) -C oracle clean
.PHONY: all libs oracle tools clean
