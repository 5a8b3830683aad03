// Unsteady nonlinear elasticity driver on the MI355X path: the reference's unsteadyNonLinElasticity test
// (feddlib/problems/tests/unsteadyNonLinElasticity/main.cpp:94-297) written against the FEDD:: operator surface -- same XML
// parameter files, same call sequence
//   structured square / cube or a .mesh file (P2 from P1) -> BCBuilder::addBC(zero Dirichlet) -> NonLinElasticity(...)
//   -> addRhsFunction(volumeY | volumeX) -> addParemeterRhs(force, ramp end, degree) -> addBoundaries -> initializeProblem
//   -> assemble -> DAESolverInTime(parameterListAll, comm) -> defineTimeStepping(1 x 1) -> setProblem -> setupTimeStepping
//   -> advanceInTime
// with "Class" = "Newmark" (DAESolverInTime::advanceInTimeNonLinearNewmark, DAESolverInTime_def.hpp:613-722): per step a Newton
// loop whose iterate, residual and update stay on the device.  Options and tail as in the other drivers: --out writes the
// displacement after the last step as text, ParaView export per step when the settings ask, the stacked-timer report.
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iomanip>

#include "feddlib/core/FEDDCore.hpp"
#include "feddlib/core/FE/Domain.hpp"
#include "feddlib/core/General/BCBuilder.hpp"
#include "feddlib/core/General/ExporterParaView.hpp"
#include "feddlib/core/Mesh/MeshPartitioner.hpp"
#include "feddlib/problems/Solver/DAESolverInTime.hpp"
#include "feddlib/problems/specific/NonLinElasticity.hpp"

// the load functions: parameters[0] is the time, parameters[1] the volume force, parameters[2] the time the load is switched
// off ("Final time force")
void rhsY2D(double* x, double* res, double* parameters) {
    res[0] = 0.;
    res[1] = parameters[0] <= parameters[2] ? parameters[1] : 0.;
}
void rhsY(double* x, double* res, double* parameters) {
    res[0] = 0.;
    res[1] = parameters[0] <= parameters[2] ? parameters[1] : 0.;
    res[2] = 0.;
}
void rhsX2D(double* x, double* res, double* parameters) {
    res[0] = parameters[0] <= parameters[2] ? parameters[1] : 0.;
    res[1] = 0.;
}
void rhsX(double* x, double* res, double* parameters) {
    res[0] = parameters[0] <= parameters[2] ? parameters[1] : 0.;
    res[1] = 0.;
    res[2] = 0.;
}
void zeroDirichlet2D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; }
void zeroDirichlet3D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; res[2] = 0.; }

typedef default_sc SC;
typedef default_lo LO;
typedef default_go GO;
typedef default_no NO;

using namespace FEDD;

int main(int argc, char* argv[]) {
    typedef Domain<SC, LO, GO, NO> Domain_Type;
    typedef Teuchos::RCP<Domain_Type> DomainPtr_Type;
    Teuchos::GlobalMPISession mpiSession(&argc, &argv);
    std::string xmlProblemFile = "parametersProblem.xml", xmlPrecFile = "parametersPrec.xml", xmlSolverFile = "parametersSolver.xml";
    std::string outFile = "solutionUnsteadyNonLinElasticity.txt";
    int volumeID = 10;
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        auto val = [&](const char* key, std::string& dst) {
            const std::string k = std::string("--") + key + "=";
            if (a.compare(0, k.size(), k) == 0) { dst = a.substr(k.size()); return true; }
            return false;
        };
        std::string vol;
        if (val("problemfile", xmlProblemFile) || val("precfile", xmlPrecFile) || val("solverfile", xmlSolverFile) || val("out", outFile)) continue;
        if (val("volumeID", vol)) { volumeID = std::stoi(vol); continue; }
        std::cerr << "unknown option " << a << std::endl;
        return 2;
    }
    try {
        Teuchos::RCP<const Teuchos::Comm<int> > comm = Teuchos::DefaultComm<int>::getComm();
        const bool verbose = comm->getRank() == 0;
        Teuchos::RCP<Teuchos::StackedTimer> stackedTimer = Teuchos::rcp(new Teuchos::StackedTimer("Unsteady nonlinear elasticity"));
        Teuchos::TimeMonitor::setStackedTimer(stackedTimer);
        ParameterListPtr_Type parameterListProblem = Teuchos::getParametersFromXmlFile(xmlProblemFile);
        ParameterListPtr_Type parameterListPrec = Teuchos::getParametersFromXmlFile(xmlPrecFile);
        ParameterListPtr_Type parameterListSolver = Teuchos::getParametersFromXmlFile(xmlSolverFile);
        ParameterListPtr_Type parameterListAll(new Teuchos::ParameterList(*parameterListProblem));
        parameterListAll->setParameters(*parameterListPrec);
        parameterListAll->setParameters(*parameterListSolver);

        int dim = parameterListProblem->sublist("Parameter").get("Dimension", 3);
        int m = parameterListProblem->sublist("Parameter").get("H/h", 5);
        std::string FEType = parameterListProblem->sublist("Parameter").get("Discretization", "P1");
        std::string meshType = parameterListProblem->sublist("Parameter").get("Mesh Type", "structured");
        std::string bcType = parameterListProblem->sublist("Parameter").get("BC Type", "volumeY");
        std::string bcPlace = parameterListProblem->sublist("Parameter").get("BC Placement", "standard");
        if (verbose) {
            std::cout << "###############################################################" << std::endl;
            std::cout << "########## Starting unsteady nonlinear elasticity ... #########" << std::endl;
            std::cout << "###############################################################" << std::endl;
        }
        DomainPtr_Type domainP1, domain;
        if (meshType == "structured") {
            if (dim == 2) {
                std::vector<double> x(2, 0.0);
                domainP1 = Teuchos::rcp(new Domain_Type(x, 1., 1., comm));
            } else {
                std::vector<double> x(3, 0.0);
                domainP1 = Teuchos::rcp(new Domain_Type(x, 1., 1., 1., comm));
            }
            domainP1->buildMesh(1, "Square", dim, "P1", 1, m, 0);
        } else if (meshType == "unstructured") {
            typedef MeshPartitioner<SC, LO, GO, NO> MeshPartitioner_Type;
            domainP1.reset(new Domain_Type(comm, dim));
            MeshPartitioner_Type::DomainPtrArray_Type domainP1Array(1);
            domainP1Array[0] = domainP1;
            ParameterListPtr_Type pListPartitioner = Teuchos::sublist(parameterListAll, "Mesh Partitioner");
            MeshPartitioner_Type partitionerP1(domainP1Array, pListPartitioner, "P1", dim);
            partitionerP1.readAndPartition(volumeID);
        } else {
            TEUCHOS_TEST_FOR_EXCEPTION(true, std::logic_error, "Mesh Type \"" + meshType + "\" is not built (structured, unstructured are)");
        }
        if (FEType == "P2") {
            domain.reset(new Domain_Type(comm, dim));
            domain->buildP2ofP1Domain(domainP1);
        } else {
            domain = domainP1;
        }

        Teuchos::RCP<BCBuilder<SC, LO, GO, NO> > bcFactory(new BCBuilder<SC, LO, GO, NO>());
        int dirichletFlag = 2;
        if (meshType == "unstructured") {
            TEUCHOS_TEST_FOR_EXCEPTION(bcPlace != "standard" && bcPlace != "foamFine", std::runtime_error, "Unknown BC Placement.");
            TEUCHOS_TEST_FOR_EXCEPTION(bcPlace == "foamFine" && dim == 2, std::runtime_error, "Foam should only be available in 3D.");
            dirichletFlag = bcPlace == "standard" ? 1 : 2;
        }
        bcFactory->addBC(dim == 2 ? zeroDirichlet2D : zeroDirichlet3D, dirichletFlag, 0, domain, "Dirichlet", dim);

        NonLinElasticity<SC, LO, GO, NO> nonLinElas(domain, FEType, parameterListAll);
        domain->info();
        nonLinElas.info();
        TEUCHOS_TEST_FOR_EXCEPTION(bcType != "volumeY" && bcType != "volumeX", std::runtime_error, "Unknown boundary function.");
        if (bcType == "volumeY") nonLinElas.addRhsFunction(dim == 2 ? rhsY2D : rhsY);
        else nonLinElas.addRhsFunction(dim == 2 ? rhsX2D : rhsX);
        double force = parameterListAll->sublist("Parameter").get("Volume force", 0.);
        double finalTimeRamp = parameterListAll->sublist("Timestepping Parameter").get("Final time force", 0.1);
        double degree = 0;
        nonLinElas.addParemeterRhs(force);
        nonLinElas.addParemeterRhs(finalTimeRamp);
        nonLinElas.addParemeterRhs(degree);

        const auto t0 = std::chrono::steady_clock::now();
        nonLinElas.addBoundaries(bcFactory);
        nonLinElas.initializeProblem();
        nonLinElas.assemble();
        fedd_timing_enable(domain->device()->ctx, 1);

        DAESolverInTime<SC, LO, GO, NO> daeTimeSolver(parameterListAll, comm);
        SmallMatrix<int> defTS(1);
        defTS[0][0] = 1;
        // (a test hook, not a reference key: a 2 x 2 definition, which the facade must refuse for this problem)
        if (parameterListProblem->sublist("Timestepping Parameter").get("Time Definition Size", 1) == 2) defTS = SmallMatrix<int>(2, 1);
        daeTimeSolver.defineTimeStepping(defTS);
        daeTimeSolver.setProblem(nonLinElas);
        daeTimeSolver.setupTimeStepping();
        daeTimeSolver.advanceInTime();
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (verbose) {
            std::cout << "time steps " << daeTimeSolver.stepsDone() << " nonlinear iterations";
            for (int k : daeTimeSolver.nonLinearIterations()) std::cout << " " << k;
            std::cout << " relres " << daeTimeSolver.getTimeProblem()->getLastRelativeResidual() << std::endl;
            std::cout << "Solve Problem " << secs << " s" << std::endl;
        }
        Teuchos::RCP<const MultiVector<SC, LO, GO, NO> > exportSolution = nonLinElas.getSolution()->getBlock(0);
        std::ofstream out(outFile);
        out << std::setprecision(17);
        auto map = exportSolution->getMap();
        auto data = exportSolution->getData(0);
        for (size_t i = 0; i < data.size(); ++i) out << map->getGlobalElement((LO)i) << " " << data[i] << "\n";
        addDeviceTimers(domain->device(), *stackedTimer);      // where the GPU time of the time loop went
        comm->barrier();
        stackedTimer->stop("Unsteady nonlinear elasticity");
        Teuchos::StackedTimer::OutputOptions options;
        options.output_fraction = options.output_histogram = options.output_minmax = true;
        if (verbose) stackedTimer->report(std::cout, comm, options);
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
