# Builds the product: librkmh_amd.so (HIP kernels + C ABI, gfx950 only) and the rkmh CLI.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH := gfx950
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-result $(EXTRA_HIPFLAGS)
CSRC := rkmh_amd/csrc
LIB := rkmh_amd/lib/librkmh_amd.so
OBJS := $(CSRC)/rk_kernels.o $(CSRC)/rk_classify.o $(CSRC)/rk_kmer.o $(CSRC)/rk_count.o $(CSRC)/rk_call.o $(CSRC)/rk_sort.o $(CSRC)/rk_fastq.o $(CSRC)/rk_fasta.o $(CSRC)/rk_inflate.o $(CSRC)/rk_api.o $(CSRC)/rk_general.o $(CSRC)/rk_route.o $(CSRC)/rk_index.o $(CSRC)/rk_counters.o $(CSRC)/rk_frontend.o $(CSRC)/rk_gunzip.o $(CSRC)/rk_packed.o $(CSRC)/rk_pack.o $(CSRC)/rk_parse.o $(CSRC)/rk_pool.o $(CSRC)/rk_parse_blocks.o $(CSRC)/rk_bgzf.o $(CSRC)/rk_format.o $(CSRC)/rk_synth.o $(CSRC)/rk_policy.o $(CSRC)/rk_pairs.o $(CSRC)/rk_pairs_host.o $(CSRC)/rk_scaled.o $(CSRC)/rk_scaled_host.o $(CSRC)/rk_gather.o $(CSRC)/rk_search.o $(CSRC)/rk_multigather.o $(CSRC)/rk_cluster.o $(CSRC)/rk_cluster_host.o $(CSRC)/rk_sample.o $(CSRC)/rk_bottom.o $(CSRC)/rk_bottom_host.o $(CSRC)/rk_screen.o $(CSRC)/rk_screen_host.o

API_DEPS := $(CSRC)/rk_api_internal.hpp $(CSRC)/rk_index_plan.hpp $(CSRC)/rk_sets.hpp $(CSRC)/rk_tile_walk.hpp $(CSRC)/rk_kernels.hpp $(CSRC)/rk_device.hpp include/rkmh_amd.h

all: $(LIB) bin/rkmh oracle

$(CSRC)/rk_kernels.o: $(CSRC)/rk_kernels.hip $(CSRC)/rk_kernels.hpp $(CSRC)/rk_device.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# the hash-space kernel: its ISA is kept under build/isa (tools/isa_blocks.py)
$(CSRC)/rk_classify.o: $(CSRC)/rk_classify.hip $(CSRC)/rk_kernels.hpp $(CSRC)/rk_device.hpp
	@mkdir -p build/isa
	cd build/isa && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
# the k-mer-space kernel: its ISA is kept next to the fused kernel's (tools/isa_blocks.py, instruction counts in DESIGN.md)
$(CSRC)/rk_kmer.o: $(CSRC)/rk_kmer.hip $(CSRC)/rk_kernels.hpp $(CSRC)/rk_device.hpp
	@mkdir -p build/isa_kmer
	cd build/isa_kmer && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_kmer && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
$(CSRC)/rk_count.o: $(CSRC)/rk_count.hip $(CSRC)/rk_kernels.hpp $(CSRC)/rk_device.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_sort.o: $(CSRC)/rk_sort.hip $(CSRC)/rk_kernels.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_fasta.o: $(CSRC)/rk_fasta.hip $(CSRC)/rk_kernels.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_fastq.o: $(CSRC)/rk_fastq.hip $(CSRC)/rk_kernels.hpp $(CSRC)/rk_filter_rule.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_inflate.o: $(CSRC)/rk_inflate.hip $(CSRC)/rk_kernels.hpp $(CSRC)/rk_crc32.hpp
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_call.o: $(CSRC)/rk_call.hip $(API_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_api.o: $(CSRC)/rk_api.hip $(API_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_general.o: $(CSRC)/rk_general.hip $(API_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_route.o: $(CSRC)/rk_route.hip $(API_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_index.o: $(CSRC)/rk_index.hip $(API_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_counters.o: $(CSRC)/rk_counters.hip $(API_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_frontend.o: $(CSRC)/rk_frontend.hip $(API_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_gunzip.o: $(CSRC)/rk_gunzip.hip $(API_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(CSRC)/rk_packed.o: $(CSRC)/rk_packed.hip $(API_DEPS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
# all-pairs sketch comparison: its ISA is kept under build/isa_pairs (tools/isa_compare.py)
$(CSRC)/rk_pairs.o: $(CSRC)/rk_pairs.hip $(API_DEPS)
	@mkdir -p build/isa_pairs
	cd build/isa_pairs && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_pairs && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
# scaled sketches: keep step and all-pairs intersection, ISA under build/isa_scaled
$(CSRC)/rk_scaled.o: $(CSRC)/rk_scaled.hip $(API_DEPS)
	@mkdir -p build/isa_scaled
	cd build/isa_scaled && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_scaled && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
# gather: the greedy decomposition of a scaled sketch, ISA under build/isa_gather
$(CSRC)/rk_gather.o: $(CSRC)/rk_gather.hip $(API_DEPS)
	@mkdir -p build/isa_gather
	cd build/isa_gather && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_gather && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
# search: the inverted index of scaled sketches and the thresholded search on it, ISA under build/isa_search
$(CSRC)/rk_search.o: $(CSRC)/rk_search.hip $(API_DEPS)
	@mkdir -p build/isa_search
	cd build/isa_search && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_search && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
# multigather: gather for a batch of queries through the inverted index, ISA under build/isa_multigather
$(CSRC)/rk_multigather.o: $(CSRC)/rk_multigather.hip $(API_DEPS)
	@mkdir -p build/isa_multigather
	cd build/isa_multigather && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_multigather && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
# cluster: hook and compress on the hits of a search, ISA under build/isa_cluster
$(CSRC)/rk_cluster.o: $(CSRC)/rk_cluster.hip $(API_DEPS)
	@mkdir -p build/isa_cluster
	cd build/isa_cluster && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_cluster && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
# the sample accumulator: fused hash-and-keep and the fold, ISA under build/isa_sample
$(CSRC)/rk_sample.o: $(CSRC)/rk_sample.hip $(API_DEPS)
	@mkdir -p build/isa_sample
	cd build/isa_sample && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_sample && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
# the cut of a bottom sample: block weights and the scan inside the crossing block, ISA under build/isa_bottom
$(CSRC)/rk_bottom.o: $(CSRC)/rk_bottom.hip $(API_DEPS)
	@mkdir -p build/isa_bottom
	cd build/isa_bottom && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_bottom && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
# screen: window hashes counted against the keys of the reference sketches, rows and owners, ISA under build/isa_screen
$(CSRC)/rk_screen.o: $(CSRC)/rk_screen.hip $(API_DEPS)
	@mkdir -p build/isa_screen
	cd build/isa_screen && $(HIPCC) $(HIPFLAGS) -save-temps -c $(CURDIR)/$< -o $(CURDIR)/$@
	@cd build/isa_screen && rm -f *.bc *.hipi *.out *.resolution.txt *.hipfb *host-x86_64*.s *.o
$(CSRC)/rk_pack.o: $(CSRC)/rk_pack.cpp $(CSRC)/rk_filter_rule.hpp include/rkmh_amd.h
	g++ -O3 -std=c++17 -fPIC -Wall -c $< -o $@
# the host read parser: pool, reader, block front end, BGZF
$(CSRC)/rk_pool.o $(CSRC)/rk_parse.o $(CSRC)/rk_parse_blocks.o $(CSRC)/rk_bgzf.o: $(CSRC)/%.o: $(CSRC)/%.cpp $(CSRC)/rk_parse_internal.hpp include/rkmh_amd.h
	g++ -O3 -std=c++17 -fPIC -Wall -c $< -o $@
$(CSRC)/rk_format.o: $(CSRC)/rk_format.cpp $(CSRC)/rk_filter_rule.hpp include/rkmh_amd.h
	g++ -O3 -std=c++17 -fPIC -Wall -c $< -o $@

$(CSRC)/rk_policy.o: $(CSRC)/rk_policy.cpp include/rkmh_amd.h
	g++ -O2 -std=c++17 -fPIC -Wall -c $< -o $@
$(CSRC)/rk_pairs_host.o: $(CSRC)/rk_pairs_host.cpp include/rkmh_amd.h
	g++ -O2 -std=c++17 -fPIC -Wall -c $< -o $@
$(CSRC)/rk_bottom_host.o: $(CSRC)/rk_bottom_host.cpp include/rkmh_amd.h
	g++ -O2 -std=c++17 -fPIC -Wall -c $< -o $@
$(CSRC)/rk_cluster_host.o: $(CSRC)/rk_cluster_host.cpp include/rkmh_amd.h
	g++ -O2 -std=c++17 -fPIC -Wall -c $< -o $@
$(CSRC)/rk_screen_host.o: $(CSRC)/rk_screen_host.cpp include/rkmh_amd.h
	g++ -O2 -std=c++17 -fPIC -Wall -c $< -o $@
$(CSRC)/rk_scaled_host.o: $(CSRC)/rk_scaled_host.cpp include/rkmh_amd.h
	g++ -O2 -std=c++17 -fPIC -Wall -pthread -c $< -o $@
$(CSRC)/rk_synth.o: $(CSRC)/rk_synth.cpp include/rkmh_amd.h
	g++ -O3 -std=c++17 -fPIC -Wall -pthread -c $< -o $@

$(LIB): $(OBJS)
	@mkdir -p rkmh_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -lz -lpthread -ldl

# the command line: one program from the rkmh_*.cpp files (what each holds: rkmh_cli.hpp)
CLI_SRCS := $(CSRC)/rkmh_main.cpp $(CSRC)/rkmh_exit.cpp $(CSRC)/rkmh_frontends.cpp $(CSRC)/rkmh_rawreads.cpp $(CSRC)/rkmh_packed.cpp $(CSRC)/rkmh_refs.cpp $(CSRC)/rkmh_classify.cpp $(CSRC)/rkmh_commands.cpp $(CSRC)/rkmh_sketch_json.cpp $(CSRC)/rkmh_sketches.cpp $(CSRC)/rkmh_sample.cpp $(CSRC)/rkmh_compare.cpp $(CSRC)/rkmh_cluster.cpp $(CSRC)/rkmh_screen.cpp $(CSRC)/rkmh_hpv16.cpp
bin/rkmh: $(CLI_SRCS) $(CSRC)/rkmh_cli.hpp $(LIB) include/rkmh_amd.h
	@mkdir -p bin
	g++ -O2 -std=c++17 -Wall -o $@ $(CLI_SRCS) -Irkmh_amd/csrc -Lrkmh_amd/lib -lrkmh_amd -Wl,-rpath,'$$ORIGIN/../rkmh_amd/lib'

oracle:
	$(MAKE) -s -C oracle

clean:
	$(RM) $(OBJS) $(LIB) bin/rkmh
	$(MAKE) -s -C oracle clean
.PHONY: all clean oracle
